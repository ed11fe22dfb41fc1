"""The generic fused-MLP kernel (mlp_fused_kernel<HT, OT>, csrc/mlp_fused.hip) and the layer-by-layer backward of an MLP with
an activation other than ReLU (functional._layerwise_mlp_backward_hip on csrc/elementwise.hip), at every width.

Every specialised forward kernel declines a multi-layer launch whose activation is not ReLU, so the cases of the family
``generic`` (tests/mlp_family_cases.py) reach the generic kernel by construction; the ReLU cases of the family are the
descriptions those kernels decline for another reason, given with the case table.  Each case runs at ``small`` (777 rows);
the cases of M.GENERIC_LOOP also run with more 128-row tiles than the persistent grid has workgroups and a ragged last tile
(``gloop``: 98,469 / 98,469 / 65,701 / 32,933 rows on 256 CUs for 1 / 2 / 4 / 8 accumulator tiles).

Instance of the dispatch switch (gnc_mlp_forward_f32) -> cases at ``small``; the case at ``gloop`` in brackets:
  <1, 1>  every shape at widths 20 and 32 (Tanh, Sigmoid, SiLU, GELU, LeakyReLU, ELU), generic_relu_narrow_node_30_5
          [generic_plain_20_Sigmoid, generic_concat_edge_32_SiLU]
  <2, 2>  plain / edge_wsplit / node / concat_edge / encoder3 at 48 and 64, generic_L2_48_SiLU  [generic_edge_wsplit_48_Sigmoid]
  <2, 1>  decoder_48_ELU, decoder5_48_LeakyReLU, decoder_64_Sigmoid, generic_relu_narrow_node_50_5  [generic_decoder_48_ELU]
  <4, 4>  plain / edge_wsplit / node / concat_edge / encoder3 at 100 and 128, the sliced and the bias-less case at 100,
          generic_relu_node_70, generic_relu_concat_edge_70  [generic_plain_100_Sigmoid]
  <4, 1>  decoder_100_Tanh, decoder_128_GELU, decoder5_128_LeakyReLU  [generic_decoder_128_GELU]
  <8, 8>  plain / edge_wsplit / node / concat_edge / encoder3 at 200 and 256, generic_L4_200_Tanh, generic_relu_node_150
          [generic_edge_wsplit_200_Sigmoid]
  <8, 1>  decoder_200_SiLU, decoder5_256_ELU, decoder_256_Sigmoid  [generic_decoder5_256_ELU]
(tests/test_mlp_family_cases_host.py asserts this coverage from M.generic_tiles.)

Sigmoid and GELU meet every padded hidden width (20, 48, 100, 200): with Sigmoid the hidden lanes beyond the width carry
act(0) = 0.5 into the next Linear, whose staged weight columns there must be zeros."""
import functools

import pytest
import torch

from tests import elementwise_cases as E
from tests import mlp_family_cases as M

DEV = "cuda:0"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from graphnet_classifier_amd import native as n
    n.load_library()
    return n


@functools.lru_cache(maxsize=None)
def _device() -> tuple:
    from graphnet_classifier_amd import native as n
    return int(n.load_library().gnc_mlp_small_batch_max_rows()), torch.cuda.get_device_properties(0).multi_processor_count


def _rows(case, key) -> int:
    small, cu = _device()
    return dict(M.generic_rows(case, small, cu), bwd=M.derived_rows(small, cu)["bwd"])[key]


def _upload(c):
    case = c["case"]
    up = {}  # the gathered segments of a shared table read ONE device tensor
    for op in c["tables"]:
        if id(op[0]) not in up:
            up[id(op[0])] = M.to_device(op, DEV)
    tabs = [up[id(op[0])] for op in c["tables"]]
    idx = {k: v.to(DEV) for k, v in c["index"].items()}
    return dict(tabs=tabs, idx=idx, segs=[(t, idx[ix] if ix else None) for t, (_, ix, _) in zip(tabs, case.segs)],
                ws=[M.to_device(w, DEV) for w in c["ws"]], bs=[b.to(DEV) if b is not None else None for b in c["bs"]],
                ln=(c["ln"][0].to(DEV), c["ln"][1].to(DEV), c["ln"][2]) if c["ln"] else None,
                residual=tabs[case.res] if case.res is not None else None, modes=case.modes if any(case.modes) else None)


def _forward(native, c, d, save=None):
    case = c["case"]
    return native.mlp_forward(d["segs"], d["ws"], d["bs"], ln=d["ln"], activation=case.activation, act_param=case.act_param,
                              residual=d["residual"], rows=c["rows"], modes=d["modes"], save_act=save)


def _err(got, want):
    return float((got.double().cpu() - want).abs().max())


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name,key", [(c.name, k) for c in M.GENERIC_CASES for k in M.generic_rows(c, 0, 1)])
def test_generic_forward_against_float64(native, name, key):
    case = M.GENERIC_BY_NAME[name]
    c = M.build(name, _rows(case, key))
    d = _upload(c)
    assert not native.small_batch_kernel_serves(d["segs"], d["ws"], d["bs"], d["ln"], case.activation, d["residual"], c["rows"],
                                                d["modes"])
    out = _forward(native, c, d)
    err = _err(out, c["out"])
    print(f"{name}/{key}: rows {c['rows']}, instance {M.generic_tiles(case)}, max-abs error vs float64 {err:.3e} (bar {c['bar']:.3e})")
    assert err < c["bar"]
    assert torch.equal(_forward(native, c, d), out)  # run-to-run determinism
    # the training forward: every kernel but the generic one writes the hidden post-activations; none here, and the same bits
    acts = []
    assert torch.equal(_forward(native, c, d, save=acts), out)
    assert acts == []


@pytest.mark.parametrize("name", [c.name for c in M.GENERIC_CASES if c.name.startswith("generic_edge_wsplit")])
def test_add_form_agrees_with_concat_form(native, name):
    """The W-split form of inference (two gathered ADD segments holding x Wa^T and x Wb^T, models/GNN.py:103-115) against the
    concat form of the same weights ([x[src] | x[dst] | e] through [Wa | Wb | We]): both within the bar of the float64
    definition of the concat form, and within that bar of each other."""
    case = M.GENERIC_BY_NAME[name]
    c = M.build(name, _rows(case, "small"))
    d, w = _upload(c), case.dims[0]
    g = torch.Generator().manual_seed(w)
    x = torch.randn(M.NODES, w, generator=g)
    bound = (3 * w) ** -0.5
    wa, wb = [(torch.rand(w, w, generator=g) * 2 - 1) * bound for _ in range(2)]
    # the ADD tables: the projections, formed in float64 and rounded once
    pa, pb = (x.double() @ wa.double().t()).float(), (x.double() @ wb.double().t()).float()
    src, dst, e = d["idx"]["src"], d["idx"]["dst"], d["tabs"][2]
    kw = dict(ln=d["ln"], activation=case.activation, act_param=case.act_param, residual=e, rows=c["rows"])
    add = native.mlp_forward([(pa.to(DEV), src), (pb.to(DEV), dst), (e, None)], d["ws"], d["bs"], modes=case.modes, **kw)
    w0 = torch.cat([wa, wb, M.view(c["ws"][0])], dim=1).to(DEV)
    xd = x.to(DEV)
    cat = native.mlp_forward([(xd, src), (xd, dst), (e, None)], [w0] + d["ws"][1:], d["bs"], **kw)
    rows64 = [x.double()[c["index"]["src"].long()], x.double()[c["index"]["dst"].long()], M.view(c["tables"][2]).double()]
    ln = (c["ln"][0].double(), c["ln"][1].double(), c["ln"][2])
    want = M.forward_def(rows64, [M.SEG_MATMUL] * 3, [w0.double().cpu()] + [M.view(t).double() for t in c["ws"][1:]],
                         [b.double() if b is not None else None for b in c["bs"]], ln, rows64[2], case.activation, case.act_param)[0]
    bar = M.TOL * max(1.0, float(want.abs().max()))
    e_add, e_cat, e_both = _err(add, want), _err(cat, want), float((add - cat).abs().max())
    print(f"{name}: ADD form {e_add:.3e}, concat form {e_cat:.3e} off float64 (bar {bar:.3e}); apart {e_both:.3e}")
    assert e_add < bar and e_cat < bar and e_both < bar


@pytest.mark.parametrize("name,param", E.ACTS)
def test_activation_inside_the_generic_kernel_on_the_table(native, name, param):
    """activate() of csrc/mlp_device.h under the bars of the row-wise kernels: two Linear layers with identity weights and no
    bias around the activation give out = act(x) exactly (products with 0 and 1, sums of one term), on the input table of
    tests/elementwise_cases.py.  With ``p * (expf(x) - 1.f)`` ELU's relative figure was 1.0 on an MI355X; with expm1f 5.6e-8."""
    x = E.table().reshape(-1, 64)
    eye = torch.eye(64, device=DEV)
    out = native.mlp_forward([(x.to(DEV), None)], [eye, eye], [None, None], activation=name, act_param=param)
    e = E.errors(out.cpu(), E.reference(x, name, param)[0], x)
    print(f"{name} inside mlp_fused_kernel<2, 2>: abs {e['abs']:.2e} of max(1, |x|) (bar {E.ABS_BAR:.0e}), rel on |x| <= "
          f"{E.REL_RANGE:.0e} {e['rel']:.2e} (bar {E.REL_BAR:.0e})")
    assert e["finite"] and e["abs"] <= E.ABS_BAR and e["rel"] <= E.REL_BAR


# ------------------------------------------------------------------------------------------------ backward, public path
def _leaf(t):
    return t.detach().requires_grad_(True)


def _run_backward(Fn, c, d, gout):
    """One forward + backward through functional.fused_mlp on fresh leaves; returns the gradients by name.  The residual is a
    leaf of its own on the storage of its segment's table (the forward recognises the pair by address), so its gradient and
    the segment's are told apart."""
    case = c["case"]
    leaves = {}
    for t in d["tabs"]:
        leaves.setdefault(t.data_ptr(), _leaf(t))
    tabs = [leaves[t.data_ptr()] for t in d["tabs"]]
    segs = [(t, d["idx"][ix] if ix else None) for t, (_, ix, _) in zip(tabs, case.segs)]
    ws, bs = [_leaf(w) for w in d["ws"]], [_leaf(b) if b is not None else None for b in d["bs"]]
    ln = (_leaf(d["ln"][0]), _leaf(d["ln"][1]), d["ln"][2]) if d["ln"] else None
    res = _leaf(d["tabs"][case.res]) if case.res is not None else None
    out = Fn.fused_mlp(segs, ws, bs, ln=ln, activation=case.activation, act_param=case.act_param, residual=res, rows=c["rows"])
    out.backward(gout)
    got = {"out": out.detach(), "tables": [t.grad for t in tabs], "dw": [w.grad for w in ws],
           "db": [b.grad if b is not None else None for b in bs]}
    if ln:
        got["dgamma"], got["dbeta"] = ln[0].grad, ln[1].grad
    if res is not None:
        got["res"] = res.grad
    return got


def _flat(got):
    return [t for v in got.values() for t in (v if isinstance(v, list) else [v]) if t is not None]


@pytest.mark.parametrize("key", M.GENERIC_BWD_KEYS)
@pytest.mark.parametrize("name", [c.name for c in M.GENERIC_BWD_CASES])
def test_generic_backward_against_float64_autograd(native, monkeypatch, name, key):
    """Table gradients (row-ordered: DX_BAR; the gathered table's, summed over its rows' edges like a weight gradient:
    DW_BAR), dW / db (DW_BAR), d gamma / d beta (LN_SUM_BAR) and the residual's gradient against float64 autograd."""
    from graphnet_classifier_amd import functional as Fn
    case = M.GENERIC_BWD_BY_NAME[name]
    c = M.build_backward(name, _rows(case, key))
    assert c["marked_share"] <= M.KINK_SHARE
    d, want, gout = _upload(c), c["grads"], c["grad_out"].to(DEV)
    calls = []
    real = Fn._layerwise_mlp_backward_hip
    monkeypatch.setattr(Fn, "_layerwise_mlp_backward_hip", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = _run_backward(Fn, c, d, gout)
    assert len(calls) == 1
    assert _err(got["out"], c["out"]) < c["bar"]
    worst = {}
    for s, (r, (w, ix, _)) in enumerate(zip(M.table_gradients(c, want, c["grad_out"]), case.segs)):
        e = _err(got["tables"][s], r)
        if ix is None:
            worst["dx"] = max(worst.get("dx", 0.0), e)
            assert e < M.DX_BAR, s
        else:
            worst["dtable"] = max(worst.get("dtable", 0.0), e / max(1.0, float(r.abs().max())))
            assert e < M.DW_BAR * max(1.0, float(r.abs().max())), s
    for l in range(len(case.dims)):
        for g, r in ((got["dw"][l], want["dw"][l]), (got["db"][l], want["db"][l])):
            if r is not None:
                rel = _err(g, r) / max(1.0, float(r.abs().max()))
                worst["dw"] = max(worst.get("dw", 0.0), rel)
                assert rel < M.DW_BAR, l
    if case.ln:
        worst["ln"] = max(_err(got["dgamma"], want["dgamma"]), _err(got["dbeta"], want["dbeta"]))
        assert worst["ln"] < M.LN_SUM_BAR
    if case.res is not None:
        assert torch.equal(got["res"], gout)
    print(f"{name}/{key}: rows {c['rows']}, " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    again = _run_backward(Fn, c, d, gout)
    assert len(calls) == 2
    for a, b in zip(_flat(got), _flat(again)):
        assert torch.equal(a, b)
