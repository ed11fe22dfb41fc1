"""The ReLU and the LayerNorm of the fused-MLP kernels, bit for bit against the PARENT of the commit that made the ReLU of
an accumulator one instruction (`v_max_f32 dst, 0, src` instead of a canonicalising v_max and the clamp).

The fixtures (tests/golden/relu_ln_bits/) were recorded by tests/golden/make_relu_ln_bits_golden.py from the parent
commit's library, selected with GNC_LIB_PATH; relu_ln_bits.json names the commit.  Outputs below 1,024 rows are stored
whole, larger ones as SHA-256 of the bytes plus every 97th row.  Every kernel that clamps accumulators is reached:

* the weights-resident kernel at 37, 4,099 and 70,007 rows: the edge encoder on computed features (EF = 1; below the
  library's limit for that form the stored features go through the same stack), the node encoder on a [rows, 3] table
  (EF = 2), a node processor, the decoder and the W-split edge processor with the fused aggregation over node tables of
  5 and of 1,000 rows;
* widths 128 and 256 at 37 and 4,099 rows (the small-batch kernel and the 16-row streaming kernel), width 128 also at
  33,001 rows, past the small-batch kernel's limit of 32,768 (the 32-row streaming kernel);
* a GraphNet of width 128 on one 144-node graph (every launch on the small-batch kernel);
* special values: plain stacks whose first Linear has zero weights and -0.0, +0.0, +-1e-40, NaN, +-1 (and, in a second
  variant, +-Inf) across its bias, so that the first ReLU sees those values; the saved post-activations show its
  result directly.  Compared as int32 like everything here: a NaN, a signed zero or a subnormal counts bit by bit.

A case also records whether the library's own query names the small-batch kernel for the launch (the edge encoder:
whether the computed-features form served it); the build under test has to route it the same way."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_split_mlp_node as node_cases
from tests.test_gpu_split_pipeline_bits import _t, _u, sha256, stored_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "relu_ln_bits")
DEV = "cuda"

pytestmark = pytest.mark.gpu

RESIDENT_ROWS = (37, 4099, 70007)
EDGE_TABLES = {"edge_t5": 5, "edge_t1000": 1000}
WIDE = {"w128": (128, (37, 4099, 33001)), "w256": (256, (37, 4099))}
# name -> (width, rows, with +-Inf): the plain stacks of the special-value case
SPECIAL = {"special64": (64, 4099, False), "special64_inf": (64, 4099, True), "special64_few": (64, 37, True),
           "special128_small": (128, 37, True), "special128": (128, 33001, True), "special256": (256, 37, True)}
KEYS = ([(name, rows) for name in ("enc_ef", "enc_n3", "node", "dec") + tuple(EDGE_TABLES) for rows in RESIDENT_ROWS] +
        [(name, rows) for name, (_, rs) in WIDE.items() for rows in rs] + [("graph144", 144)] +
        [(name, rows) for name, (_, rows, _) in SPECIAL.items()])


def _ln(rng, width):
    return (rng.uniform(0.5, 1.5, (width,)).astype(np.float32), rng.uniform(-0.5, 0.5, (width,)).astype(np.float32))


def _stack(rng, dims):
    return ([_u(rng, a, (b, a)) for a, b in zip(dims[:-1], dims[1:])], [_u(rng, a, (b,)) for a, b in zip(dims[:-1], dims[1:])])


def special_bias(width, with_inf):
    vals = [-0.0, 0.0, 1e-40, -1e-40, float("nan"), 1.0, -1.0] + ([float("inf"), -float("inf")] if with_inf else [])
    return np.array([vals[j % len(vals)] for j in range(width)], dtype=np.float32)


def _family(native, segs, ws, bs, ln, residual, rows, modes=None, vector_rows=True):
    """Whether the library's query names the small-batch kernel for this launch ("small-batch") or not ("other": the
    weights-resident kernel up to width 64, a streaming kernel above)."""
    lib = native.load_library()
    s, w, b, res, rows, _ = native._prepare_mlp(segs, ws, bs, residual, rows, modes, vector_rows=vector_rows)
    dummy = torch.empty(max(rows, 1), w[-1].size(0), device=DEV)
    desc = native.make_mlp_desc(s, w, b, ln, "ReLU", 0.0, res, dummy, rows)
    return "small-batch" if lib.gnc_mlp_small_batch_supported(ctypes.byref(desc)) == 0 else "other"


def run_case(native, name, rows):
    """({tensor name: CPU tensor}, routing answer or None) of one case.  Shared with tests/golden/make_relu_ln_bits_golden.py."""
    rng = np.random.default_rng(9000 + 17 * [k[0] for k in KEYS].index(name) + rows % 991)
    got, family = {}, None
    if name in ("enc_ef", "enc_n3"):
        nodes = 20011
        x = rng.standard_normal((rows, 3)).astype(np.float32)
        pos = rng.standard_normal((nodes, 2)).astype(np.float32)
        src, dst = rng.integers(0, nodes, rows).astype(np.int32), np.sort(rng.integers(0, nodes, rows)).astype(np.int32)
        ws, bs = _stack(rng, [3, 64, 64, 64])
        g, b = _ln(rng, 64)
        ws, bs, ln = [_t(w) for w in ws], [_t(v) for v in bs], (_t(g), _t(b), 1e-5)
        if name == "enc_ef":
            out = native.mlp_forward_edge_features(_t(pos), _t(src), _t(dst), ws, bs, ln=ln)
            family = "resident" if out is not None else "stored features"
            if out is None:  # the caller's other arm (MLP.forward_edge_features returned None)
                out = native.mlp_forward([(native.edge_features(_t(pos), _t(src), _t(dst)), None)], ws, bs, ln=ln)
            got["out"] = out
        else:
            family = _family(native, [(_t(x), None)], ws, bs, ln, None, rows, vector_rows=False)
            got["out"] = native.mlp_forward([(_t(x), None)], ws, bs, ln=ln, rows=rows)
    elif name in ("node", "dec"):
        which = {"node": "node_res", "dec": "dec1"}[name]
        c = node_cases._case(which, rows)
        x, ws, bs = _t(c["x"]), [_t(w) for w in c["ws"]], [_t(v) for v in c["bs"]]
        segs = [(x, None), (_t(c["agg"]), None)] if name == "node" else [(x, None)]
        ln = (_t(c["ln"][0]), _t(c["ln"][1]), 1e-5) if name == "node" else None
        res = x if name == "node" else None
        family = _family(native, segs, ws, bs, ln, res, rows)
        got["out"] = native.mlp_forward(segs, ws, bs, ln=ln, residual=res)
    elif name in EDGE_TABLES:
        nodes = EDGE_TABLES[name]
        x = rng.standard_normal((rows, 64)).astype(np.float32)
        ps, pd = rng.standard_normal((nodes, 64)).astype(np.float32), rng.standard_normal((nodes, 64)).astype(np.float32)
        src, dst = rng.integers(0, nodes, rows).astype(np.int32), np.sort(rng.integers(0, nodes, rows)).astype(np.int32)
        ws, bs = _stack(rng, [64, 64, 64, 64])
        g, b = _ln(rng, 64)
        x, ws, bs, ln, dst = _t(x), [_t(w) for w in ws], [_t(v) for v in bs], (_t(g), _t(b), 1e-5), _t(dst)
        segs = [(_t(ps), _t(src)), (_t(pd), dst), (x, None)]
        modes = [native.SEG_ADD, native.SEG_ADD, native.SEG_MATMUL]
        family = _family(native, segs, ws, bs, ln, x, rows, modes)
        rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV),
                            torch.cumsum(torch.bincount(dst.long(), minlength=nodes), 0)]).int()
        kw = dict(ln=ln, residual=x, rows=rows, modes=modes, aggregate=(dst, rowptr, nodes))
        got["out"], got["agg"] = native.mlp_forward(segs, ws, bs, **kw)
        assert got["agg"] is not None, "the fused aggregation did not serve this shape"
        only = native.mlp_forward(segs, ws, bs, agg_only=True, **kw)  # (the aggregate-only instance where it serves the shape)
        got["only_agg"] = only[1]
    elif name in WIDE:
        width = WIDE[name][0]
        x = _t(rng.standard_normal((rows, width)).astype(np.float32))
        ws, bs = _stack(rng, [width, width, width, width])
        g, b = _ln(rng, width)
        ws, bs, ln = [_t(w) for w in ws], [_t(v) for v in bs], (_t(g), _t(b), 1e-5)
        family = _family(native, [(x, None)], ws, bs, ln, x, rows)
        got["out"] = native.mlp_forward([(x, None)], ws, bs, ln=ln, residual=x)
    elif name == "graph144":
        from graphnet_classifier_amd import synthetic
        from graphnet_classifier_amd.GNN import GraphNet
        from graphnet_classifier_amd.topology import clear_topology_cache
        batch = synthetic.superpixel_like_graphs(1, seed=1000, shapes=((12, 12),))
        assert batch.num_nodes == rows
        torch.manual_seed(0)
        model = GraphNet(**synthetic.graphnet_kwargs(128, 2)).to(DEV).eval()
        clear_topology_cache()
        with torch.no_grad():
            got["out"] = model(batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV))
    else:
        width, _, with_inf = SPECIAL[name]
        x = rng.standard_normal((rows, width)).astype(np.float32)
        x[::2] = -np.abs(x[::2])  # (rows of one sign: the zero products of such a row all carry the same sign)
        x[1::2] = np.abs(x[1::2])
        ws, bs = _stack(rng, [width, width, width, width])
        ws[0][:] = 0.0
        bs[0] = special_bias(width, with_inf)
        ws[1] = np.eye(width, dtype=np.float32)
        bs[1][:] = 0.0
        x, ws, bs = _t(x), [_t(w) for w in ws], [_t(v) for v in bs]
        family = _family(native, [(x, None)], ws, bs, None, None, rows)
        acts = []
        got["out"] = native.mlp_forward([(x, None)], ws, bs)
        got["save_out"] = native.mlp_forward([(x, None)], ws, bs, save_act=acts)
        for l, a in enumerate(acts):
            got[f"save_act{l}"] = a
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}, family


def fixture_path(name, rows):
    return os.path.join(GOLDEN, f"{name}_{rows}.npz")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "relu_ln_bits.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name,rows", KEYS)
def test_bits_match_parent(meta, name, rows):
    from graphnet_classifier_amd import native
    native.load_library()
    got, family = run_case(native, name, rows)
    want_meta = meta["cases"][f"{name}/{rows}"]
    assert family == want_meta["family"], "another kernel family than the parent's serves this launch"
    assert sorted(got) == sorted(want_meta["tensors"])
    with np.load(fixture_path(name, rows)) as z:
        want = {k: torch.from_numpy(z[k]) for k in z.files}
    for k in sorted(got):
        g, w = stored_rows(got[k]), want[k]
        assert list(got[k].shape) == want_meta["tensors"][k]["shape"] and g.shape == w.shape and g.dtype == w.dtype == torch.float32
        differ = int((g.view(torch.int32) != w.view(torch.int32)).sum())
        digest = sha256(got[k])
        print(f"{name}/{rows} [{family}] {k}: {differ} of {g.numel()} stored values differ from the parent's; sha256 "
              f"{'equal' if digest == want_meta['tensors'][k]['sha256'] else 'DIFFERS'}")
        assert differ == 0, k
        assert digest == want_meta["tensors"][k]["sha256"], k
    if name in SPECIAL:  # what today's pair of instructions does and one v_max has to keep: NaN -> 0, nothing below zero
        a0 = got["save_act0"]
        assert not torch.isnan(a0).any() and bool((a0 >= 0).all())
        width, _, with_inf = SPECIAL[name]
        bias = torch.from_numpy(special_bias(width, with_inf))
        assert torch.equal(a0[:, bias == 1.0], torch.ones_like(a0[:, bias == 1.0]))
        if with_inf:
            assert bool(torch.isposinf(a0[:, torch.isposinf(bias)]).all()) and bool((a0[:, torch.isneginf(bias)] == 0).all())
