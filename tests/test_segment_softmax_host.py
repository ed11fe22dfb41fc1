"""Host-only checks of the attention neighbourhood aggregation (K21): the C ABI (declared, exported, argument checks answered
without a GPU), the float64 reference of tests/segment_softmax_cases.py on a hand-written example, the seed conditions of its error
bars and of tests/test_gpu_attention_aggregation_model.py, and the ``aggregation="attention"`` argument of the constructors."""
import os
import re
import subprocess

import pytest
import torch

from tests import segment_softmax_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gnc_segment_softmax_csr_f32", "gnc_segment_softmax_backward_f32", "gnc_segment_softmax_weights_f32")


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
    assert lib.gnc_abi_version() == native.ABI_VERSION == 20  # added without an ABI bump
    with open(os.path.join(ROOT, "graphnet_classifier_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS\s*=.*\bsegment_softmax\.hip\b", f.read(), re.M)
    for fn in ("segment_softmax_csr", "segment_softmax_backward", "segment_softmax_weights"):
        assert callable(getattr(native, fn))


def test_argument_checks_answer_without_a_gpu():
    """GNC_REQUIRE runs in front of any launch: null pointers, negative sizes and a short leading dimension are refused with a
    message; empty problems return GNC_OK."""
    from graphnet_classifier_amd import native
    lib = native.load_library()
    p = 1 << 12  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before a launch
    fwd, bwd, wts = lib.gnc_segment_softmax_csr_f32, lib.gnc_segment_softmax_backward_f32, lib.gnc_segment_softmax_weights_f32
    # forward: (src, ld_src, scores, rowptr, perm, num_nodes, num_edges, feat_dim, out, ld_out, saved, stream)
    assert fwd(p, 8, p, None, None, 4, 10, 8, p, 8, p, None) != 0 and b"null" in lib.gnc_last_error_string()    # rowptr
    assert fwd(p, 8, p, p, None, 4, 10, 8, None, 8, p, None) != 0                                                # out
    assert fwd(p, 8, p, p, None, 4, 10, 8, p, 8, None, None) != 0                                                # saved
    assert fwd(None, 8, p, p, None, 4, 10, 8, p, 8, p, None) != 0                                                # src
    assert fwd(p, 8, None, p, None, 4, 10, 8, p, 8, p, None) != 0 and b"scores" in lib.gnc_last_error_string()  # scores
    assert fwd(p, 8, p, p, None, -1, 10, 8, p, 8, p, None) != 0 and b"negative" in lib.gnc_last_error_string()
    assert fwd(p, 8, p, p, None, 4, -1, 8, p, 8, p, None) != 0
    assert fwd(p, 4, p, p, None, 4, 10, 8, p, 8, p, None) != 0 and b"leading" in lib.gnc_last_error_string()
    assert fwd(p, 8, p, p, None, 4, 10, 8, p, 4, p, None) != 0
    assert fwd(p + 2, 8, p, p, None, 4, 10, 8, p, 8, p, None) != 0 and b"aligned" in lib.gnc_last_error_string()
    assert fwd(None, 8, None, None, None, 0, 0, 8, None, 8, None, None) == 0  # no nodes
    assert fwd(None, 8, None, None, None, 4, 0, 0, None, 8, None, None) == 0  # no columns
    # backward: (grad_out, ld_grad, src, ld_src, scores, out, ld_out, saved, dst_of_row, N, E, D, grad_src, ld_gsrc, grad_scores, s)
    good = [p, 8, p, 8, p, p, 8, p, p, 4, 10, 8, p, 8, p, None]
    for slot in (0, 2, 4, 5, 7, 8, 12, 14):
        bad = list(good)
        bad[slot] = None
        assert bwd(*bad) != 0 and b"null" in lib.gnc_last_error_string(), slot
    for slot in (1, 3, 6, 13):
        bad = list(good)
        bad[slot] = 7
        assert bwd(*bad) != 0 and b"leading" in lib.gnc_last_error_string(), slot
    assert bwd(*(good[:9] + [-1] + good[10:])) != 0 and bwd(*(good[:10] + [-1] + good[11:])) != 0
    assert bwd(*(good[:9] + [0] + good[10:])) != 0 and b"destination" in lib.gnc_last_error_string()  # rows without a node
    assert bwd(None, 8, None, 8, None, None, 8, None, None, 4, 0, 8, None, 8, None, None) == 0  # no rows
    # weights: (scores, saved, dst_of_row, num_rows, alpha, stream)
    assert wts(None, p, p, 10, p, None) != 0 and wts(p, None, p, 10, p, None) != 0 and wts(p, p, None, 10, p, None) != 0
    assert wts(p, p, p, 10, None, None) != 0 and wts(p, p, p, -1, p, None) != 0
    assert wts(None, None, None, 0, None, None) == 0


def test_the_reference_on_a_hand_written_example():
    src, scores, index, out, alpha = C.hand_example()
    assert C.degrees(index, 5).tolist() == [2, 3, 2, 0, 1]
    got, got_alpha, m, z = C.ref_attention(src, scores, index, 5)
    assert got.dtype == torch.float64 and torch.allclose(got, out, rtol=0, atol=1e-15)
    assert torch.allclose(got_alpha, alpha, rtol=0, atol=1e-15)
    assert torch.equal(got[3], torch.zeros(2, dtype=torch.float64)) and float(m[3]) == 0.0 and float(z[3]) == 0.0   # empty
    assert torch.equal(got[4], src[5].double()) and float(z[4]) == 1.0 and float(m[4]) == -2.0                         # single row
    assert torch.equal(got[1], C.R.ref_mean(src, index, 5)[1]) and float(z[1]) == 3.0 and float(m[1]) == 3.25           # equal scores
    assert float(got_alpha[7]) == 0.0 and torch.equal(got[2], src[3].double())                                          # -inf: nothing
    sums = torch.zeros(5, dtype=torch.float64).index_add_(0, index, got_alpha)
    assert torch.allclose(sums, torch.tensor([1.0, 1, 1, 0, 1], dtype=torch.float64), rtol=0, atol=1e-15)
    assert torch.allclose(C.ref_weighted_abs(src, scores, index, 5)[0], torch.tensor([2.5, 4.0], dtype=torch.float64), rtol=0, atol=1e-15)
    # the backward against float64 autograd of the same formulas
    grad = torch.arange(10.0).reshape(5, 2) + 1
    s = scores.clone().requires_grad_(True)
    x = src.double().requires_grad_(True)
    e = torch.exp(s - m[index])
    a = e / torch.zeros(5, dtype=torch.float64).index_add(0, index, e)[index]
    torch.zeros(5, 2, dtype=torch.float64).index_add(0, index, a[:, None] * x).backward(grad.double())
    g_src, g_score = C.ref_attention_backward(grad, src, scores, index, 5)
    assert torch.allclose(g_src, x.grad, rtol=0, atol=1e-14) and torch.allclose(g_score, s.grad, rtol=0, atol=1e-13)
    assert float(g_score[5]) == 0.0 and float(g_score[7]) == 0.0  # a single row's score, and a weight of zero, move nothing
    # one NaN score: its destination's row is NaN, every other row is what it was
    bad = scores.clone()
    bad[4] = float("nan")
    nan_out, nan_alpha, nan_m, _ = C.ref_attention(src, bad, index, 5)
    assert bool(torch.isnan(nan_out[1]).all()) and float(nan_m[1]) == 3.25
    keep = torch.tensor([0, 2, 3, 4])
    assert torch.equal(nan_out[keep], got[keep]) and bool(torch.isnan(nan_alpha[index == 1]).all())
    # the fp32 evaluation and the oracle stand-in agree with the reference
    f_out, f_alpha = C.fp32_attention(src, scores.float(), index, 5)
    assert torch.allclose(f_out.double(), out, rtol=0, atol=1e-6) and torch.allclose(f_alpha.double(), alpha, rtol=0, atol=1e-6)


def test_small_cases_have_the_degrees_and_the_bars_are_finite():
    index = C.small_index()
    assert index.numel() == 211 and set(C.degrees(index, C.SMALL_N).tolist()) == {0, 1, 3, 4, 5, 9, 70}
    deg, dmax, c = C.error_constants(C.scores_for(C.SMALL_E, 8, seed=0), index, C.SMALL_N)
    assert torch.equal(c, 2 * deg + 2 * dmax + 12) and float(dmax.max()) > 8 and bool((dmax[deg <= 1] == 0).all())


@pytest.mark.parametrize("width", C.BACKWARD_WIDTHS)
def test_seed_condition_fp32_evaluation_stays_within_half_of_each_bar(width):
    """The project's seed-condition pattern: an fp32 torch evaluation of the same formulas on the CPU uses at most HALF of every
    bar on every small case (if a case fails this, the case changes, not the bar)."""
    for scale in C.SCALES:
        index, src, scores, grad = C.small_case(width, scale)
        n = C.SMALL_N
        out, alpha, _, _ = C.ref_attention(src, scores, index, n)
        g_src, g_score = C.ref_attention_backward(grad, src, scores, index, n)
        b = C.bars(src, scores, index, n, grad)
        f_out, f_alpha = C.fp32_attention(src, scores, index, n)
        f_src, f_score = C.fp32_attention_backward(grad, src, scores, index, n)
        used = {"forward": C.fraction((f_out.double() - out).abs(), b["forward"]),
                "alpha": C.fraction((f_alpha.double() - alpha).abs(), b["alpha"]),
                "grad_src": C.fraction((f_src.double() - g_src).abs(), b["grad_src"]),
                "grad_score": C.fraction((f_score.double() - g_score).abs(), b["grad_score"])}
        print(f"D={width} scale={scale}: fraction of the bars used by fp32 torch {used}")
        assert all(v <= 0.5 for v in used.values()), (width, scale, used)


def _kwargs():
    from graphnet_classifier_amd import synthetic
    return synthetic.graphnet_kwargs(32, 3, out_channels=8)


def test_attention_reaches_every_node_processor_and_adds_four_tensors_per_block():
    from graphnet_classifier_amd.GNN import AGGREGATIONS, GraphNet, NodeProcessor
    assert AGGREGATIONS == ("sum", "mean", "max", "attention")
    torch.manual_seed(0)
    base = GraphNet(**_kwargs())
    torch.manual_seed(0)
    g = GraphNet(**_kwargs(), aggregation="attention")
    nodes = [m for m in g.modules() if isinstance(m, NodeProcessor)]
    assert len(nodes) == 3 and all(m.aggregation == "attention" for m in nodes)
    assert g.aggregation == g.graph_processor.aggregation == "attention" and len(list(g.buffers())) == 0
    extra = [k for k in g.state_dict() if k not in base.state_dict()]
    want = [f"graph_processor.blocks.{b}.node_model.gate.model.{i}.{w}" for b in range(3) for i in (0, 2) for w in ("weight", "bias")]
    assert extra == want and [k for k in g.state_dict() if k not in extra] == list(base.state_dict())
    sd = g.state_dict()
    assert tuple(sd[want[0]].shape) == (32, 32) and tuple(sd[want[2]].shape) == (1, 32) and tuple(sd[want[3]].shape) == (1,)
    # keys in module order: the gate sits BEHIND node_processor
    keys = list(sd)
    assert keys.index(want[0]) > max(i for i, k in enumerate(keys) if k.startswith("graph_processor.blocks.0.node_model.node_processor"))
    g16 = GraphNet(**_kwargs(), aggregation="attention", attention_hidden=16)
    assert tuple(g16.state_dict()[want[0]].shape) == (16, 32)
    # block 0's shared tensors draw the numbers they draw without the gate (its gate is built behind its node_processor)
    for k, v in base.state_dict().items():
        if k.startswith(("node_encoder", "edge_encoder", "graph_processor.blocks.0.")):
            assert torch.equal(v, sd[k]), k


def test_the_old_modes_keep_their_state_dicts_and_their_random_draws():
    from graphnet_classifier_amd.GNN import GraphNet
    torch.manual_seed(0)
    base = GraphNet(**_kwargs())
    for mode in ("sum", "mean", "max"):
        torch.manual_seed(0)
        sd = GraphNet(**_kwargs(), aggregation=mode).state_dict()
        assert list(sd) == list(base.state_dict()) and not any("gate" in k for k in sd)
        assert all(torch.equal(v, base.state_dict()[k]) for k, v in sd.items())


def test_attention_hidden_with_another_mode_raises():
    from graphnet_classifier_amd.GNN import GraphNet, GraphProcessor, NodeProcessor, build_GN_block
    makers = (lambda **k: NodeProcessor(8, 8, **k), lambda **k: build_GN_block(8, 8, **k), lambda **k: GraphProcessor(2, 8, 8, **k),
              lambda **k: GraphNet(**_kwargs(), **k))
    for make in makers:
        for mode in ("sum", "mean", "max"):
            with pytest.raises(ValueError, match="attention_hidden"):
                make(aggregation=mode, attention_hidden=16)
        with pytest.raises(ValueError, match="attention_hidden"):
            make(attention_hidden=16)
        with pytest.raises(ValueError, match="sum.*mean.*max"):
            make(aggregation="softmax")
        make(aggregation="attention", attention_hidden=16)
        make(aggregation="attention")
    with pytest.raises(ValueError):
        NodeProcessor(8, 8, aggregation="attention", attention_hidden=0)


def test_a_sum_checkpoint_loads_with_strict_false_and_leaves_the_gates_alone():
    from graphnet_classifier_amd.GNN import GraphNet
    torch.manual_seed(1)
    ckpt = GraphNet(**_kwargs()).state_dict()
    torch.manual_seed(2)
    g = GraphNet(**_kwargs(), aggregation="attention")
    before = {k: v.clone() for k, v in g.state_dict().items()}
    res = g.load_state_dict(ckpt, strict=False)
    assert not res.unexpected_keys and len(res.missing_keys) == 12 and all(".node_model.gate." in k for k in res.missing_keys)
    for k, v in g.state_dict().items():
        assert torch.equal(v, before[k] if ".gate." in k else ckpt[k]), k
    with pytest.raises(RuntimeError):
        g.load_state_dict(ckpt, strict=True)


def test_seed_conditions_of_the_model_tests(monkeypatch):
    from tests import test_gpu_attention_aggregation_model as T
    figures = T.seed_conditions(monkeypatch)
    print(figures)
    assert figures["fp32_vs_f64"] <= 0.5 * T.BAR, figures
    assert figures["vs_mean"] > 200 * T.BAR, figures  # condition 2
