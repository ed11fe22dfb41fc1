"""Host-only checks of the mean / max neighbourhood aggregation (K18): the C ABI (declared, exported, argument checks answered
without a GPU), the ``aggregation`` argument of the four constructors, the CPU reference of tests/segment_reduce_cases.py on a
hand-written example, and the seed conditions of tests/test_gpu_aggregation_model.py."""
import os
import re
import subprocess

import pytest
import torch

from tests import segment_reduce_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gnc_segment_reduce_csr_f32", "gnc_segment_reduce_backward_f32", "gnc_rows_div_degree_f32")


def test_library_exports_the_launches_and_the_header_declares_them():
    from graphnet_classifier_amd import native
    lib = native.load_library()
    with open(os.path.join(ROOT, "include", "gnc_hip.h")) as f:
        header = f.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gnc_[a-z0-9_]+)", nm))
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported
    for name, value in (("MEAN", native.SEGMENT_MEAN), ("MAX", native.SEGMENT_MAX)):
        assert re.search(rf"#define\s+GNC_SEGMENT_{name}\s+{value}\b", header)
    assert lib.gnc_abi_version() == native.ABI_VERSION  # added without an ABI bump
    with open(os.path.join(ROOT, "graphnet_classifier_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS\s*=.*\bsegment_reduce\.hip\b", f.read(), re.M)


def test_argument_checks_answer_without_a_gpu():
    """GNC_REQUIRE runs in front of any launch: a bad mode, argmax with MEAN, negative sizes and a short leading dimension are
    refused with status GNC_ERR_INVALID_ARGUMENT and a message; empty problems return GNC_OK."""
    from graphnet_classifier_amd import native
    lib = native.load_library()
    p = 1 << 12  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before a launch
    fwd, bwd, div = lib.gnc_segment_reduce_csr_f32, lib.gnc_segment_reduce_backward_f32, lib.gnc_rows_div_degree_f32
    assert fwd(p, 8, p, None, 4, 10, 8, 3, p, 8, None, None) != 0 and b"mode" in lib.gnc_last_error_string()
    assert fwd(p, 8, p, None, 4, 10, 8, native.SEGMENT_MEAN, p, 8, p, None) != 0 and b"argmax" in lib.gnc_last_error_string()
    assert fwd(p, 8, p, None, -1, 10, 8, native.SEGMENT_MAX, p, 8, None, None) != 0
    assert fwd(p, 4, p, None, 4, 10, 8, native.SEGMENT_MAX, p, 8, None, None) != 0 and b"leading" in lib.gnc_last_error_string()
    assert fwd(p, 8, None, None, 4, 10, 8, native.SEGMENT_MAX, p, 8, None, None) != 0
    assert fwd(None, 8, None, None, 0, 0, 8, native.SEGMENT_MAX, None, 8, None, None) == 0  # no nodes
    assert bwd(p, 8, p, p, None, 4, 10, 8, native.SEGMENT_MAX, p, 8, None) != 0 and b"argmax" in lib.gnc_last_error_string()
    assert bwd(p, 8, p, None, None, 4, 10, 8, native.SEGMENT_MEAN, p, 8, None) != 0
    assert bwd(p, 8, p, p, p, 4, 10, 8, 0, p, 8, None) != 0
    assert bwd(None, 8, None, None, None, 4, 0, 8, native.SEGMENT_MEAN, None, 8, None) == 0  # no rows
    assert div(p, 4, p, 4, 8, None) != 0 and div(None, 8, p, 4, 8, None) != 0 and div(None, 8, None, 0, 8, None) == 0
    for bad in ("sum", "min", 0):
        with pytest.raises(ValueError):
            native._segment_mode(bad)


def _kwargs():
    from graphnet_classifier_amd import synthetic
    return synthetic.graphnet_kwargs(32, 3, out_channels=8)


def test_aggregation_reaches_every_node_processor_and_leaves_the_state_dict_alone():
    from graphnet_classifier_amd.GNN import GraphNet, NodeProcessor
    shapes = None
    for mode in ("sum", "mean", "max"):
        torch.manual_seed(0)
        g = GraphNet(**_kwargs(), aggregation=mode)
        nodes = [m for m in g.modules() if isinstance(m, NodeProcessor)]
        assert len(nodes) == 3 and all(m.aggregation == mode for m in nodes) and g.aggregation == mode
        assert g.graph_processor.aggregation == mode
        sd = {k: tuple(v.shape) for k, v in g.state_dict().items()}
        shapes = shapes or sd
        assert list(sd.items()) == list(shapes.items()) and not any("aggregation" in k for k in sd)
        assert len(list(g.buffers())) == 0
    torch.manual_seed(0)
    default = GraphNet(**_kwargs())
    assert default.aggregation == "sum" and all(m.aggregation == "sum" for m in default.modules() if isinstance(m, NodeProcessor))
    assert GraphNet().aggregation == "sum"
    for mode in ("mean", "max"):  # a checkpoint of one mode loads strictly into another
        GraphNet(**_kwargs(), aggregation=mode).load_state_dict(default.state_dict(), strict=True)


def test_an_unknown_aggregation_raises_at_each_constructor():
    from graphnet_classifier_amd.GNN import GraphNet, GraphProcessor, NodeProcessor, build_GN_block
    makers = (lambda a: NodeProcessor(8, 8, aggregation=a), lambda a: build_GN_block(8, 8, aggregation=a),
              lambda a: GraphProcessor(0, 8, 8, aggregation=a), lambda a: GraphProcessor(2, 8, 8, aggregation=a),
              lambda a: GraphNet(**_kwargs(), aggregation=a))
    for make in makers:
        for bad in ("bogus", "Mean", None, "add"):
            with pytest.raises(ValueError, match="sum.*mean.*max"):
                make(bad)
        for good in ("sum", "mean", "max"):
            make(good)
    assert NodeProcessor(8, 8).aggregation == "sum" and build_GN_block(8, 8).node_model.aggregation == "sum"


def test_the_reference_on_a_hand_written_example():
    src, index, mean, mx, arg = C.hand_example()
    assert C.degrees(index, 5).tolist() == [2, 3, 1, 0, 1]
    got_mean = C.ref_mean(src, index, 5)
    assert got_mean.dtype == torch.float64 and torch.equal(got_mean, mean)
    got_max, got_arg = C.ref_max(src, index, 5)
    assert torch.equal(got_max.view(torch.int32), mx.view(torch.int32))  # bits: the tie of -0.0 and +0.0 keeps the first, -0.0
    assert torch.equal(got_arg, arg) and bool(torch.signbit(got_max[1, 1]))
    grad = torch.arange(10.0).reshape(5, 2) + 1
    gm = C.ref_mean_backward(grad, index, 5)
    assert torch.equal(gm[1], grad[1].double() / 3) and torch.equal(gm[4], gm[1]) and torch.equal(gm[5], grad[4].double())
    gx = C.ref_max_backward(grad, index, arg)
    want = torch.zeros(7, 2)
    want[2], want[1], want[3], want[5] = grad[0], grad[1], grad[2], grad[4]
    assert torch.equal(gx, want) and not bool(torch.signbit(gx).any())
    # a NaN wins its column, at its first row
    src[4, 0] = float("nan")
    src[6, 0] = float("nan")
    nan_max, nan_arg = C.ref_max(src, index, 5)
    assert bool(torch.isnan(nan_max[1, 0])) and int(nan_arg[1, 0]) == 4 and int(nan_arg[1, 1]) == 1
    # the oracle stand-ins agree with the reference and are differentiable
    src, index, mean, mx, arg = C.hand_example()
    s = src.double().requires_grad_(True)
    assert torch.allclose(C.oracle_scatter_mean(s, index, 5), mean, rtol=0, atol=1e-15)
    out = C.oracle_scatter_max(s, index, 5)
    assert torch.equal(out.detach(), mx.double())
    out.backward(grad.double())
    assert torch.equal(s.grad, want.double())
    assert C.min_top2_gap(src, index, 5) == 0.0  # the tie


def test_small_regime_case_has_the_degrees_the_kernels_need():
    index = C.small_index()
    deg = C.degrees(index, C.SMALL_N)
    assert index.numel() == 211 and set(deg.tolist()) == {0, 1, 3, 4, 5, 9, 70}
    assert not bool((index[1:] >= index[:-1]).all())  # unsorted


def test_seed_conditions_of_the_model_tests(monkeypatch):
    from tests import test_gpu_aggregation_model as T
    figures = T.seed_conditions(monkeypatch)
    print(figures)
    for mode in T.MODES:
        assert figures[mode]["fp32_vs_f64"] <= 0.5 * T.BAR, (mode, figures[mode])  # condition 1
    assert figures["max"]["selections"] == 8 and figures["max"]["min_gap"] > T.MIN_GAP, figures["max"]  # condition 2
