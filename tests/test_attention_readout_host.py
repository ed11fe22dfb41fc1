"""Host-only checks of the attention read-out (K19): the C ABI (declared, exported, bound with the signatures of ``native.py``), the
host walk of the kernels' index arithmetic (tools/attention_pool_index_check.cpp over csrc/attention_pool_index.h and
csrc/pool_index.h, compiled with the address and undefined-behaviour sanitizers), and ``CombinedModel(readout="attention")``."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gnc_graph_attention_pool_workspace_floats": (ctypes.c_int64, 3), "gnc_graph_attention_pool_forward_f32": (ctypes.c_int32, 12),
         "gnc_graph_attention_pool_backward_f32": (ctypes.c_int32, 14), "gnc_graph_attention_weights_f32": (ctypes.c_int32, 7)}


def test_library_exports_the_attention_launches_and_the_header_declares_them():
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
    assert lib.gnc_abi_version() == native.ABI_VERSION  # added without an ABI bump
    with open(os.path.join(ROOT, "graphnet_classifier_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS\s*=.*\battention_pool\.hip\b", f.read(), re.M)
    for fn in ("graph_attention_pool_forward", "graph_attention_pool_backward", "graph_attention_weights"):
        assert callable(getattr(native, fn))


def test_workspace_follows_the_pooling_plan_without_a_gpu():
    """The regime is K17's plan: no workspace for many graphs, ``slots * (C + 1)`` floats in the split regime, -1 outside the set."""
    from graphnet_classifier_amd import native
    ws = native.load_library().gnc_graph_attention_pool_workspace_floats
    for rows, C, G in ((6400, 64, 64), (16384, 128, 1), (32768, 128, 1), (718, 3, 9), (1280, 130, 1), (0, 8, 3)):
        plan = native.graph_pool_plan(rows, C, G)
        assert ws(rows, C, G) == (plan["slots"] * (C + 1) if plan["split"] else 0), (rows, C, G)
    assert ws(16384, 128, 1) > 0 and ws(6400, 64, 64) == 0
    assert ws(100, 0, 1) == -1 and ws(100, 8, 0) == -1 and ws(1 << 31, 8, 1) == -1


def test_index_arithmetic_on_the_host(tmp_path):
    """Every (workgroup, thread) of the forward launches of both regimes, of the backward launch and of the weights launch,
    enumerated on the host over batches with empty graphs, exact multiples of the chunk length, slack rows and offsets outside the
    table: no address leaves its buffer, every row of a graph is read exactly once, every workspace slot the merge reads was
    written.  The walker is a host program of its own, so it runs under the address and undefined-behaviour sanitizers."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    out = str(tmp_path / "attention_pool_index_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "graphnet_classifier_amd", "csrc"), os.path.join(ROOT, "tools", "attention_pool_index_check.cpp"),
                    "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and "attention_pool_index_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_combined_model_attention_readout_argument():
    import torch
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    from graphnet_classifier_amd.MLP import MLP
    kw = synthetic.graphnet_kwargs(32, 1, out_channels=8)

    def build(readout, **extra):
        torch.manual_seed(0)
        return CombinedModel(GraphNet(**kw), num_nodes=12, classes=3, readout=readout, **extra)

    att = build("attention")
    assert "attention" in CombinedModel.READOUTS
    assert att.classifier.fc1.in_features == 8 and att.pooled and att.ragged_readout is True and att.readout == "attention"
    assert isinstance(att.gate, MLP) and att.gate.norm_type is None
    gate_keys = [k for k in att.state_dict() if k.startswith("gate.")]
    assert gate_keys == ["gate.model.0.weight", "gate.model.0.bias", "gate.model.2.weight", "gate.model.2.bias"]
    assert tuple(att.gate.model[0].weight.shape) == (32, 8) and tuple(att.gate.model[2].weight.shape) == (1, 32)
    # the other five read-outs: no gate, the same keys as each other
    keys = None
    for readout in ("flatten", "mean", "max", "sum", "hybrid"):
        m = build(readout)
        assert not hasattr(m, "gate") and not any(k.startswith("gate") for k in m.state_dict())
        keys = keys or list(m.state_dict())
        assert list(m.state_dict()) == keys
    assert [k for k in att.state_dict() if not k.startswith("gate.")] == keys
    # built after the classifier: under one seed every non-gate tensor is the mean model's, bit for bit
    mean = build("mean").state_dict()
    for k, v in att.state_dict().items():
        if not k.startswith("gate."):
            assert torch.equal(v, mean[k]), k
    wide = build("attention", gate_hidden=5)
    assert tuple(wide.gate.model[0].weight.shape) == (5, 8) and tuple(wide.gate.model[2].weight.shape) == (1, 5)
    with pytest.raises(ValueError):
        build("mean", gate_hidden=32)
    with pytest.raises(ValueError):
        build("bogus")
    with pytest.raises(TypeError):
        CombinedModel(GraphNet(**kw), 12, 3, "attention", 32)  # keyword-only
    # a checkpoint of another pooled read-out loads with strict=False and leaves the gate at its initialisation
    before = {k: v.clone() for k, v in att.state_dict().items() if k.startswith("gate.")}
    torch.manual_seed(1)
    other = CombinedModel(GraphNet(**kw), num_nodes=12, classes=3, readout="max").state_dict()
    missing = att.load_state_dict(other, strict=False)
    assert sorted(missing.missing_keys) == sorted(before) and not missing.unexpected_keys
    assert all(torch.equal(att.state_dict()[k], v) for k, v in before.items())
    assert torch.equal(att.state_dict()["classifier.fc1.weight"], other["classifier.fc1.weight"])
    with pytest.raises(ValueError):
        build("mean").attention_weights(torch.zeros(4, 3), torch.zeros(4, 2), torch.zeros(2, 0, dtype=torch.long))
