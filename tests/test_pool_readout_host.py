"""Host-only checks of the global pooling read-out (K17): the C ABI (declared, exported, the plan answered without a GPU), the
host walk of the kernels' index arithmetic (tools/pool_index_check.cpp over csrc/pool_index.h), and ``CombinedModel``'s
``readout`` argument."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gnc_graph_pool_plan", "gnc_graph_pool_forward_f32", "gnc_graph_pool_backward_f32")


def test_library_exports_the_pooling_launches_and_the_header_declares_them():
    from graphnet_classifier_amd import native
    lib = native.load_library()
    with open(os.path.join(ROOT, "include", "gnc_hip.h")) as f:
        header = f.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gnc_[a-z0-9_]+)", nm))
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported
    for name, bit in (("SUM", native.POOL_SUM), ("MEAN", native.POOL_MEAN), ("MAX", native.POOL_MAX)):
        assert re.search(rf"#define\s+GNC_POOL_{name}\s+{bit}\b", header)
    assert lib.gnc_abi_version() == native.ABI_VERSION  # added without an ABI bump
    with open(os.path.join(ROOT, "graphnet_classifier_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS\s*=.*\bpool_readout\.hip\b", f.read(), re.M)


def test_plan_answers_without_a_gpu():
    from graphnet_classifier_amd import native
    plan = native.graph_pool_plan
    many, split = plan(6400, 64, 64), plan(16384, 128, 1)
    R = many["chunk_rows"]
    assert R > 0 and split["chunk_rows"] == R
    assert many["split"] == 0 and many["workspace_floats"] == 0          # 64 superpixel graphs of ~100 rows
    assert split["split"] == 1                                            # one 128 x 128 pixel graph
    # the split regime's workspace holds (sum, max, argmax) per chunk and column: it grows with rows / chunk_rows
    assert split["slots"] >= 16384 // R and split["workspace_floats"] == 3 * split["slots"] * 128
    twice = plan(32768, 128, 1)
    assert twice["split"] == 1 and twice["slots"] - split["slots"] == 16384 // R
    assert twice["workspace_floats"] > split["workspace_floats"]
    # the tiling is a function of the width alone (it fixes the summation order), and covers it
    for C in (1, 3, 4, 64, 128, 130, 256):
        a, b = plan(718, C, 9), plan(10 * R, C, 1)
        assert a["split"] == 0 and b["split"] == 1
        for k in ("vec", "col_lanes", "row_lanes", "col_tiles", "chunk_rows"):
            assert a[k] == b[k], (C, k)
        assert a["col_lanes"] * a["row_lanes"] == 256 and a["vec"] == (4 if C % 4 == 0 else 1)
        assert a["col_tiles"] * a["col_lanes"] * a["vec"] >= C > (a["col_tiles"] - 1) * a["col_lanes"] * a["vec"]
    assert plan(10_000 * 150, 128, 10_000)["split"] == 0                  # many small graphs
    assert plan(0, 8, 3) is not None and plan(0, 8, 3)["split"] == 0      # no rows at all: every graph is empty
    assert plan(100, 0, 1) is None and plan(100, 8, 0) is None and plan(1 << 31, 8, 1) is None


def test_index_arithmetic_on_the_host(tmp_path):
    """Every (workgroup, thread) of the forward launches and every item of the backward launch, enumerated on the host over
    batches with empty graphs, exact multiples of the chunk length, slack rows and offsets outside the table: no address leaves
    its buffer, every element of a graph is read exactly once, the merge reads exactly the slots that were written."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    out = str(tmp_path / "pool_index_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "graphnet_classifier_amd", "csrc"),
                    os.path.join(ROOT, "tools", "pool_index_check.cpp"), "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and "pool_index_check: ok" in r.stdout, r.stdout[-2000:]


def test_combined_model_readout_argument():
    import torch
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    kw = synthetic.graphnet_kwargs(32, 1, out_channels=8)
    with pytest.raises(ValueError):
        CombinedModel(GraphNet(**kw), num_nodes=12, classes=2, readout="bogus")
    keys = None
    for readout, width, ragged in (("flatten", 12 * 8, False), ("mean", 8, True), ("max", 8, True), ("sum", 8, True), ("hybrid", 24, True)):
        torch.manual_seed(0)
        m = CombinedModel(GraphNet(**kw), num_nodes=12, classes=3, readout=readout)
        assert m.classifier.fc1.in_features == width and m.classifier.fc3.out_features == 3
        assert m.readout == readout and m.num_nodes == 12 and m.ragged_readout is ragged and m.pooled is ragged
        keys = keys or list(m.state_dict())
        assert list(m.state_dict()) == keys and not any("readout" in k for k in keys)
    torch.manual_seed(0)
    default = CombinedModel(GraphNet(**kw), num_nodes=12, classes=3)
    assert default.readout == "flatten" and default.ragged_readout is False
    with pytest.raises(TypeError):
        CombinedModel(GraphNet(**kw), 12, 3, "mean")  # keyword-only
