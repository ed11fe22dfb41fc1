"""Host-only checks of the capacity-padded top-K pooling (K20, ``pool_padded=True``): the C ABI of the two padded launches, the host
walk of the slack arithmetic (tools/topk_pool_padded_index_check.cpp over csrc/topk_pool_index.h, compiled with the address and
undefined-behaviour sanitizers and run as a program of its own), the reference layout of tests/topk_pool_padded_cases.py on a
hand-written example, and the constructor rules of ``GraphNet(pool_padded=True)``."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import topk_pool_padded_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gnc_topk_pool_select_padded_f32": ("gnc_topk_pool_select_f32", 10),
         "gnc_topk_pool_filter_edges_padded": ("gnc_topk_pool_filter_edges", 16)}
GNC_ERR_INVALID_ARGUMENT = -1


def test_library_exports_the_padded_launches_and_the_header_declares_them():
    from graphnet_classifier_amd import native
    lib = native.load_library()
    with open(os.path.join(ROOT, "include", "gnc_hip.h")) as f:
        header = f.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gnc_[a-z0-9_]+)", nm))
    for name, (sized, nargs) in NAMES.items():
        declared = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert declared, name
        assert len(declared.group(1).split(",")) == nargs, name
        assert name in native.EXPORTED_SYMBOLS and name in exported
        fn = getattr(lib, name)
        # the padded form takes the sized form's arguments
        assert fn.restype is ctypes.c_int32 and tuple(fn.argtypes) == tuple(native._SIGNATURES[name][1]) == tuple(native._SIGNATURES[sized][1])
    assert lib.gnc_abi_version() == native.ABI_VERSION == 20  # added without an ABI bump


def test_argument_checks_answer_without_a_launch():
    from graphnet_classifier_amd import native
    lib = native.load_library()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    sel, flt = lib.gnc_topk_pool_select_padded_f32, lib.gnc_topk_pool_filter_edges_padded
    ws = lib.gnc_topk_pool_edge_workspace_ints
    for ratio in (0.0, 1.5, float("nan")):
        assert sel(p, p, 1, 4, ratio, p, p, p, p, None) == GNC_ERR_INVALID_ARGUMENT, ratio
    assert sel(p, p, 1, 4, 0.5, p, p, p, None, None) == GNC_ERR_INVALID_ARGUMENT       # null counts
    assert sel(p, p, 1, 1 << 31, 0.5, p, p, p, p, None) == GNC_ERR_INVALID_ARGUMENT    # rows >= 2^31
    assert flt(p, p, p, 8, 4, p, p, p, p, p, p, p, p, p, ws(8) - 1, None) == GNC_ERR_INVALID_ARGUMENT   # workspace too small
    assert flt(p, p, p, 8, 4, p, p, None, p, p, p, p, p, p, ws(8), None) == GNC_ERR_INVALID_ARGUMENT    # null counts
    assert flt(None, p, p, 8, 4, p, p, p, p, p, p, p, p, p, ws(8), None) == GNC_ERR_INVALID_ARGUMENT    # null src
    # no rows: no row a slack edge could loop on, so the padded filter launches nothing and answers GNC_OK on the host
    assert flt(p, p, p, 8, 0, p, p, p, p, p, p, p, p, p, ws(8), None) == 0


def test_slack_arithmetic_on_the_host(tmp_path):
    """Every (workgroup, thread) that writes a tail - the slack self-loops, the slack rows' offsets, ``kept`` behind N' - over rows, E,
    N', E' from {0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 70001} and sampled positions near 2^31 / 4 and 2^31, in a host program of
    its own under the address and undefined-behaviour sanitizers."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    out = str(tmp_path / "topk_pool_padded_index_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "graphnet_classifier_amd", "csrc"), "-I", os.path.join(ROOT, "tools"),
                    os.path.join(ROOT, "tools", "topk_pool_padded_index_check.cpp"), "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and "topk_pool_padded_index_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_the_padded_reference_on_a_hand_written_example():
    nan, inf = float("nan"), float("inf")
    # the example of tests/test_topk_pool_host.py: graph 0 = rows 1..6, graph 1 empty, graph 2 = rows 6..11; rows 0 and 12 of no graph
    s = np.array([9.0, 0.5, -0.0, 0.5, 0.0, nan, -inf, 2.0, 2.0, 2.0, nan, 1.0, 7.0], dtype=np.float32)
    src = np.array([1, 3, 0, 2, 3, 5, 9, 7, 8, 40, 9], dtype=np.int32)
    dst = np.array([1, 1, 2, 3, 3, 3, 7, 8, 9, 9, 12], dtype=np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=13))]).astype(np.int32)
    r = P.ref_padded(s, [1, 7, 7, 12], 0.5, src, dst, rowptr)
    assert r["n_out"] == 6 and r["e_out"] == 7 and r["graph_ptr"].tolist() == [0, 3, 3, 6]
    assert r["kept"].tolist() == [1, 2, 3, 7, 8, 9] + [-1] * 7
    assert r["kept_edges"].tolist() == [0, 1, 3, 4, 6, 7, 8] + [-1] * 4
    # S_R = 7 slack rows 6 ... 12, S_E = 4 slack edges: edge t loops on 6 + floor(7 t / 4) = 6, 7, 9, 11
    assert r["src"].tolist() == [0, 2, 1, 2, 5, 3, 4, 6, 7, 9, 11] and r["dst"].tolist() == [0, 0, 2, 2, 3, 4, 5, 6, 7, 9, 11]
    # rowptr'[6 + u] = 7 + ceil(4 u / 7) = 7, 8, 9, 9, 10, 10, 11, 11
    assert r["rowptr"].tolist() == [0, 2, 2, 4, 5, 6, 7, 8, 9, 9, 10, 10, 11, 11]
    assert np.array_equal(np.bincount(r["dst"], minlength=13), np.diff(r["rowptr"]))  # the CSR offsets describe the list
    # nodes only
    assert set(P.ref_padded(s, [1, 7, 7, 12], 0.5)) == {"new_id", "kept", "graph_ptr", "n_out"}
    # ratio 1 over all rows and an edge with an endpoint outside the table: S_R = 0, the one slack edge loops on the last row
    r = P.ref_padded(np.arange(4, dtype=np.float32), [0, 4], 1.0, np.array([0, 9, 2], np.int32), np.array([1, 1, 3], np.int32),
                     np.array([0, 0, 2, 2, 3], np.int32))
    assert r["n_out"] == 4 and r["e_out"] == 2 and r["src"].tolist() == [0, 2, 3] and r["dst"].tolist() == [1, 3, 3]
    assert r["rowptr"].tolist() == [0, 0, 1, 1, 3] and r["kept_edges"].tolist() == [0, 2, -1]


def _kw():
    from graphnet_classifier_amd import synthetic
    return synthetic.graphnet_kwargs(32, 3, out_channels=8)


def test_graphnet_padded_pooling_arguments_and_state_dict():
    from graphnet_classifier_amd.GNN import (CombinedModel, GraphNet, TopKPool, pooling_prevents_capture, pooling_reads_sizes_back,
                                             uses_node_pooling)
    kw = _kw()

    def build(**extra):
        torch.manual_seed(0)
        return GraphNet(**kw, **extra)

    sized, padded = build(pool_ratio=0.5), build(pool_ratio=0.5, pool_padded=True)
    assert not sized.pool_padded and padded.pool_padded and padded.pooling and padded.pool_after == (0, 1, 2)
    assert build(pool_ratio=0.5, pool_padded=False).pool_padded is False and build().pool_padded is False
    # no parameter, no key: under one seed every tensor is the sized model's
    assert list(padded.state_dict()) == list(sized.state_dict())
    assert all(torch.equal(v, padded.state_dict()[k]) for k, v in sized.state_dict().items())
    pools = list(padded.graph_processor.pools.values())
    assert len(pools) == 3 and all(isinstance(p, TopKPool) and p.padded for p in pools)
    assert all(not p.padded for p in sized.graph_processor.pools.values())
    assert TopKPool(8, 0.5).padded is False and TopKPool(8, 0.5, 4, padded=True).padded is True
    assert padded.pooled_nodes(69) == sized.pooled_nodes(69) == 9
    # the predicates: both models pool, only the sized one reads sizes back
    assert uses_node_pooling(sized) and uses_node_pooling(padded) and not uses_node_pooling(build())
    assert pooling_reads_sizes_back(sized) and not pooling_reads_sizes_back(padded) and not pooling_reads_sizes_back(build())
    mean = CombinedModel(padded, num_nodes=16, classes=2, readout="mean")
    assert uses_node_pooling(mean) and not pooling_reads_sizes_back(mean) and not pooling_prevents_capture(mean)
    # a capture takes padded pooling under a pooled read-out alone; an un-pooled model is not concerned
    assert pooling_prevents_capture(padded) and pooling_prevents_capture(CombinedModel(padded, num_nodes=padded.pooled_nodes(16), classes=2))
    assert pooling_prevents_capture(CombinedModel(sized, num_nodes=16, classes=2, readout="mean")) and not pooling_prevents_capture(build())
    with pytest.raises(ValueError, match="pool_padded"):
        build(pool_padded=True)  # without pool_ratio
    with pytest.raises(NotImplementedError, match="BatchNorm1d"):
        torch.manual_seed(0)
        GraphNet(**{**kw, "norm_type": "BatchNorm1d"}, pool_ratio=0.5, pool_padded=True)
    torch.manual_seed(0)
    assert GraphNet(**{**kw, "norm_type": "BatchNorm1d"}, pool_ratio=0.5).pooling  # the sized form keeps BatchNorm
    # the wrappers take the flag
    from graphnet_classifier_amd import functional as Fn, native
    import inspect
    assert inspect.signature(Fn.topk_pool).parameters["padded"].default is False
    for fn in (native.topk_pool_select, native.topk_pool_filter_edges):
        assert inspect.signature(fn).parameters["padded"].default is False
    # nothing in the padded path reads a device value on the host
    source = inspect.getsource(native.topk_pool_select) + inspect.getsource(native.topk_pool_filter_edges)
    assert ".item()" not in source and ".tolist()" not in source
