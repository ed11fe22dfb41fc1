"""Host-only checks of the top-K node pooling (K20): the C ABI (declared, exported, bound with the signatures of ``native.py``), the
argument checks that answer in front of any launch, the host walk of the kernels' index arithmetic (tools/topk_pool_index_check.cpp
over csrc/topk_pool_index.h, compiled with the address and undefined-behaviour sanitizers), the reference of
tests/topk_pool_cases.py on hand-written examples, the constructor rules of ``GraphNet(pool_ratio=...)`` and the conditions on the
inputs of tests/test_gpu_topk_pool_model.py (asserted in the float64 reference alone)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import topk_pool_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gnc_topk_pool_select_f32": (ctypes.c_int32, 10), "gnc_topk_pool_edge_workspace_ints": (ctypes.c_int64, 1),
         "gnc_topk_pool_filter_edges": (ctypes.c_int32, 16), "gnc_topk_pool_rows_forward_f32": (ctypes.c_int32, 10),
         "gnc_topk_pool_rows_backward_f32": (ctypes.c_int32, 13)}
GNC_ERR_INVALID_ARGUMENT = -1


def test_library_exports_the_pooling_launches_and_the_header_declares_them():
    from graphnet_classifier_amd import native
    lib = native.load_library()
    with open(os.path.join(ROOT, "include", "gnc_hip.h")) as f:
        header = f.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gnc_[a-z0-9_]+)", nm))
    for name, (restype, nargs) in NAMES.items():
        declared = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert declared, name
        assert len(declared.group(1).split(",")) == nargs, name  # the header's parameter count is the binding's
        assert name in native.EXPORTED_SYMBOLS and name in exported
        fn = getattr(lib, name)
        assert fn.restype is restype and len(fn.argtypes) == nargs and tuple(fn.argtypes) == tuple(native._SIGNATURES[name][1])
    assert lib.gnc_abi_version() == native.ABI_VERSION == 20  # added without an ABI bump
    with open(os.path.join(ROOT, "graphnet_classifier_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS\s*=.*\btopk_pool\.hip\b", f.read(), re.M)
    for fn in ("topk_pool_select", "topk_pool_filter_edges", "topk_pool_rows_forward", "topk_pool_rows_backward"):
        assert callable(getattr(native, fn))
    from graphnet_classifier_amd import functional as Fn
    from graphnet_classifier_amd.topology import GraphTopology
    assert callable(Fn.topk_pool) and callable(GraphTopology.from_sorted)


def test_argument_checks_answer_without_a_launch():
    """Every call below is refused by a GNC_REQUIRE in front of the first launch (no device is needed to be refused), and the
    workspace query is plain host arithmetic."""
    from graphnet_classifier_amd import native
    lib = native.load_library()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    sel, flt = lib.gnc_topk_pool_select_f32, lib.gnc_topk_pool_filter_edges
    fwd, bwd = lib.gnc_topk_pool_rows_forward_f32, lib.gnc_topk_pool_rows_backward_f32
    for ratio in (0.0, -0.5, 1.5, float("nan")):
        assert sel(p, p, 1, 4, ratio, p, p, p, p, None) == GNC_ERR_INVALID_ARGUMENT, ratio
    assert b"ratio" in lib.gnc_last_error_string()
    assert sel(p, p, 0, 4, 0.5, p, p, p, p, None) == GNC_ERR_INVALID_ARGUMENT          # no graph
    assert sel(p, p, 1, -1, 0.5, p, p, p, p, None) == GNC_ERR_INVALID_ARGUMENT         # negative rows
    assert sel(p, p, 1, 1 << 31, 0.5, p, p, p, p, None) == GNC_ERR_INVALID_ARGUMENT    # rows >= 2^31
    assert sel(None, p, 1, 4, 0.5, p, p, p, p, None) == GNC_ERR_INVALID_ARGUMENT       # null scores
    assert sel(p, p, 1, 4, 0.5, p, p, p, None, None) == GNC_ERR_INVALID_ARGUMENT       # null counts
    assert sel(p, p + 4, 1, 4, 0.5, p, p, p, p, None) == GNC_ERR_INVALID_ARGUMENT      # graph_ptr not 8-byte aligned
    assert b"aligned" in lib.gnc_last_error_string()
    ws = lib.gnc_topk_pool_edge_workspace_ints
    assert ws(0) == 0 and ws(1) == 2 and ws(K.EDGE_TILE) == K.EDGE_TILE + 1 and ws(K.EDGE_TILE + 1) == K.EDGE_TILE + 3
    assert ws(-1) == -1 and ws(1 << 31) == -1
    assert flt(p, p, p, 8, 4, p, p, p, p, p, p, p, p, p, ws(8) - 1, None) == GNC_ERR_INVALID_ARGUMENT   # workspace too small
    assert b"workspace" in lib.gnc_last_error_string()
    assert flt(p, p, p, 8, 4, p, p, None, p, p, p, p, p, p, ws(8), None) == GNC_ERR_INVALID_ARGUMENT    # null counts
    assert flt(None, p, p, 8, 4, p, p, p, p, p, p, p, p, p, ws(8), None) == GNC_ERR_INVALID_ARGUMENT    # null src
    assert flt(p, p, p, -1, 4, p, p, p, p, p, p, p, p, p, ws(8), None) == GNC_ERR_INVALID_ARGUMENT      # negative E
    assert fwd(p, 3, 4, 8, p, 2, None, p, 8, None) == GNC_ERR_INVALID_ARGUMENT         # ld_x < C
    assert b"leading dimension" in lib.gnc_last_error_string()
    assert fwd(p, 8, 4, 8, p, 5, None, p, 8, None) == GNC_ERR_INVALID_ARGUMENT         # more kept rows than rows
    assert fwd(p, 8, 4, 0, p, 2, None, p, 8, None) == GNC_ERR_INVALID_ARGUMENT         # C = 0
    assert fwd(None, 8, 4, 8, p, 2, None, p, 8, None) == GNC_ERR_INVALID_ARGUMENT      # null x
    assert bwd(p, 8, 2, p, 8, p, p, 4, 8, None, 8, None, None) == GNC_ERR_INVALID_ARGUMENT   # no gradient wanted
    assert bwd(p, 8, 2, p, 8, None, p, 4, 8, p, 8, p, None) == GNC_ERR_INVALID_ARGUMENT      # ds without a gate
    assert bwd(p, 8, 2, p, 8, p, p, 4, 8, p, 7, None, None) == GNC_ERR_INVALID_ARGUMENT      # ld_dx < C
    # empty problems are GNC_OK without a launch
    assert fwd(p, 8, 4, 8, p, 0, None, p, 8, None) == 0 and bwd(p, 8, 0, p, 8, p, p, 0, 8, p, 8, p, None) == 0
    # the Python wrappers refuse a ratio outside (0, 1] before they look at a tensor
    for ratio in (0, 0.0, -1, 1.0001, float("nan"), None, "0.5", True):
        with pytest.raises(ValueError):
            native.topk_pool_select(torch.zeros(3), torch.tensor([0, 3]), ratio)


def test_index_arithmetic_on_the_host(tmp_path):
    """Every (workgroup, thread) of the select, edge-scan and row launches over the awkward sizes, in a host program of its own
    under the address and undefined-behaviour sanitizers: no address leaves its buffer, each input is read once and each output
    written once, the radix walk keeps what a stable sort keeps, the key map is monotone with ``-0.0 == +0.0`` and NaN lowest.  The
    program also prints ``keep_count`` for the pairs where ``ratio * n`` is an integer in exact arithmetic: they must be Python's
    ``math.ceil(ratio * n)``."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    out = str(tmp_path / "topk_pool_index_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "graphnet_classifier_amd", "csrc"), os.path.join(ROOT, "tools", "topk_pool_index_check.cpp"),
                    "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and "topk_pool_index_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    printed = {(float(a), int(b)): int(c) for a, b, c in re.findall(r"keep_count (\S+) (\d+) = (\d+)", r.stdout)}
    for ratio, n in K.CEIL_PAIRS + ((1e-3, 16384), (0.5, 1), (1.0, 7)):
        assert printed[(ratio, n)] == min(n, max(1, math.ceil(ratio * n))) == K.keep_count(ratio, n), (ratio, n)
    assert printed[(0.25, 0)] == 0


def test_the_reference_on_a_hand_written_example():
    from graphnet_classifier_amd import native
    nan, inf = float("nan"), float("inf")
    #                 graph 0: rows 1..6                      | graph 1: rows 6..6 | graph 2: rows 6..11
    s = np.array([9.0, 0.5, -0.0, 0.5, 0.0, nan, -inf, 2.0, 2.0, 2.0, nan, 1.0, 7.0], dtype=np.float32)
    gp = [1, 7, 7, 12]
    new_id, kept, out = K.ref_select(s, gp, 0.5)
    # graph 0 (n = 6, k = 3): 0.5 (row 1), 0.5 (row 3), then the zeros tie -> the lower row 2 (-0.0 == +0.0)
    # graph 2 (n = 5, k = 3): 2.0 x 3 (rows 7, 8, 9); rows 0 and 12 belong to no graph
    assert kept.tolist() == [1, 2, 3, 7, 8, 9] and out.tolist() == [0, 3, 3, 6]
    assert new_id.tolist() == [-1, 0, 1, 2, -1, -1, -1, 3, 4, 5, -1, -1, -1]
    # ratio 1: everything inside a graph, NaN included; a tiny ratio: one row per non-empty graph
    assert K.ref_select(s, gp, 1.0)[1].tolist() == list(range(1, 12))
    assert K.ref_select(s, gp, 1e-3)[1].tolist() == [1, 7] and K.ref_select(s, gp, 1e-3)[2].tolist() == [0, 1, 1, 2]
    # NaN ranks below -inf: of [nan, -inf] one row is kept, and it is -inf
    assert K.ref_select(np.array([nan, -inf], np.float32), [0, 2], 0.5)[1].tolist() == [1]
    assert K.ref_select(np.array([nan, nan, nan], np.float32), [0, 3], 0.5)[1].tolist() == [0, 1]  # ties of NaN by row
    for ratio, n in K.CEIL_PAIRS:
        assert K.keep_count(ratio, n) == native.topk_keep_count(ratio, n) == math.ceil(ratio * n)
    assert [K.keep_count(r, n) for r, n in K.CEIL_PAIRS] == [1, 7, 3, 3]
    assert K.keep_count(1e-3, 5) == 1 and K.keep_count(1.0, 5) == 5 and K.keep_count(0.5, 0) == 0
    # the edge filter on the first result: dst-sorted edges (src, dst)
    src = np.array([1, 3, 0, 2, 3, 5, 9, 7, 8, 40, 9], dtype=np.int32)
    dst = np.array([1, 1, 2, 3, 3, 3, 7, 8, 9, 9, 12], dtype=np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=13))]).astype(np.int32)
    s2, d2, ke, eid, rp = K.ref_filter(src, dst, rowptr, new_id)
    assert ke.tolist() == [0, 1, 3, 4, 6, 7, 8]  # (0 -> 2), (5 -> 3), (40 -> 9: outside) and (9 -> 12) go
    assert s2.tolist() == [0, 2, 1, 2, 5, 3, 4] and d2.tolist() == [0, 0, 2, 2, 3, 4, 5]
    assert eid.tolist() == [0, 1, -1, 2, 3, -1, 4, 5, 6, -1, -1] and rp.tolist() == [0, 2, 2, 4, 5, 6, 7]
    # gate and backward in float64
    x = np.arange(26, dtype=np.float64).reshape(13, 2)
    out_rows, dx, ds = K.ref_rows(x, s.astype(np.float64), kept, grad=np.ones((6, 2)))
    t = math.tanh(0.5)
    assert float((out_rows[0] - torch.tensor([2 * t, 3 * t], dtype=torch.float64)).abs().max()) < 1e-15
    assert float((dx[1] - t).abs().max()) < 1e-15 and dx[0].tolist() == [0.0, 0.0]
    assert abs(float(ds[1]) - (1 - t * t) * 5.0) < 1e-15 and float(ds[4]) == 0.0


def _kw():
    from graphnet_classifier_amd import synthetic
    return synthetic.graphnet_kwargs(32, 3, out_channels=8)


def test_graphnet_pooling_arguments_and_state_dict():
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet, TopKPool, uses_node_pooling
    from graphnet_classifier_amd.MLP import MLP
    kw = _kw()

    def build(**extra):
        torch.manual_seed(0)
        return GraphNet(**kw, **extra)

    plain, none = build(), build(pool_ratio=None)
    assert list(plain.state_dict()) == list(none.state_dict()) and not none.pooling and none.pool_after == ()
    assert not hasattr(none.graph_processor, "pools") and not uses_node_pooling(none) and none.pooled_nodes(69) == 69
    assert all(torch.equal(v, none.state_dict()[k]) for k, v in plain.state_dict().items())
    pooled = build(pool_ratio=0.5)
    assert pooled.pooling and pooled.pool_ratio == 0.5 and pooled.pool_after == (0, 1, 2) and uses_node_pooling(pooled)
    pool_keys = [k for k in pooled.state_dict() if ".pools." in k]
    assert pool_keys == [f"graph_processor.pools.{i}.gate.model.{j}.{w}" for i in range(3) for j in (0, 2) for w in ("weight", "bias")]
    assert [k for k in pooled.state_dict() if ".pools." not in k] == list(plain.state_dict())
    # constructed last: every other parameter is the un-pooled model's, bit for bit, under one seed
    assert all(torch.equal(v, pooled.state_dict()[k]) for k, v in plain.state_dict().items())
    pool = pooled.graph_processor.pools["1"]
    assert isinstance(pool, TopKPool) and isinstance(pool.gate, MLP) and pool.gate.norm_type is None and pool.ratio == 0.5
    assert tuple(pool.gate.model[0].weight.shape) == (32, 32) and tuple(pool.gate.model[2].weight.shape) == (1, 32)
    some = build(pool_ratio=0.25, pool_after=[2, 0], pool_hidden=5)
    assert some.pool_after == (0, 2) and sorted(some.graph_processor.pools) == ["0", "2"]
    assert tuple(some.graph_processor.pools["2"].gate.model[0].weight.shape) == (5, 32)
    assert some.pooled_nodes(100) == 7 and pooled.pooled_nodes(69) == 9 and pooled.pooled_nodes(1) == 1 and pooled.pooled_nodes(0) == 0
    assert build(pool_ratio=1).pooled_nodes(33) == 33
    for bad in ({"pool_ratio": 0.0}, {"pool_ratio": 1.5}, {"pool_ratio": -0.1}, {"pool_ratio": "half"}, {"pool_after": [0]},
                {"pool_hidden": 16}, {"pool_ratio": 0.5, "pool_after": [3]}, {"pool_ratio": 0.5, "pool_after": [-1]},
                {"pool_ratio": 0.5, "pool_after": [1, 1]}, {"pool_ratio": 0.5, "pool_after": [0.0]}, {"pool_ratio": 0.5, "pool_hidden": 0}):
        with pytest.raises(ValueError):
            build(**bad)
    # the read-outs: a pooled GraphNet under a flatten read-out needs graph_ptr in the num_graphs form
    m = CombinedModel(pooled, num_nodes=pooled.pooled_nodes(16), classes=2)
    assert m.classifier.fc1.in_features == 2 * 8
    with pytest.raises(ValueError, match="kept_nodes"):
        CombinedModel(plain, num_nodes=4, classes=2).kept_nodes(torch.zeros(4, 3), torch.zeros(4, 2), torch.zeros(2, 0, dtype=torch.long))


def test_from_sorted_rejects_what_is_not_a_device_csr():
    from graphnet_classifier_amd.topology import GraphTopology
    z = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError):
        GraphTopology.from_sorted(z, z, z, 2, z, False)  # host tensors
    with pytest.raises(ValueError):
        GraphTopology.from_sorted(z.long(), z, z, 2, z, False)


def test_seed_conditions_of_the_model_tests():
    """Conditions (a) - (c) on the inputs of tests/test_gpu_topk_pool_model.py, in the float64 reference alone (figures: DESIGN.md,
    K20): at every pooling layer and graph the gap between the k-th and the (k + 1)-th score is at least 100 x the measured |fp32
    oracle - float64 oracle| of the scores, the kept set is not the first k rows, and the pooled logits differ from the un-pooled
    model's by at least ten bars."""
    from tests import test_gpu_topk_pool_model as M
    for fig in M.seed_condition_figures():
        print(fig)
        assert fig["min_gap"] >= 100.0 * fig["score_err"], fig
        assert not fig["first_k"], fig
        assert fig["apart"] >= 1e-4, fig
