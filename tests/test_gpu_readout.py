"""GPU: the single-graph read-out kernels (csrc/readout.hip) called directly through ``native.readout_forward`` /
``native.readout_backward`` and held to float64 at the shapes of tests/readout_cases.py - every loop boundary of both kernels,
both fc1 paths by layout, NULL biases, ``need_dy=False``, the ReLU edges and NaN, the ticket counter across back-to-back
launches, a second stream and a graph replay, the width limits, and the autograd surface (``functional.readout``,
``LinearClassifier``).  Bars: per case and per output, 4 x max(error of the fp32 CPU evaluation, 2^-23 max|ref|)
(tests/readout_cases.py; proven on the host in tests/test_readout_host.py).  Before every call the caching allocator is primed
with freed NaN-filled blocks of the outputs' sizes, so an element the kernel never wrote shows."""
import itertools

import pytest
import torch

from tests import readout_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
LAYOUT_SHAPE = (1028, 128, 32, 2)  # F % 4 == 0: the layout alone chooses the fc1 path


def _dev(c):
    return {k: None if v is None else v.float().to(DEV) for k, v in c.items()}


def _prime(*sizes):
    """What torch.empty hands the next call: freed blocks full of NaN, one per output."""
    blocks = [torch.full((max(int(n), 1),), NAN, device=DEV) for n in sizes]
    del blocks


def _forward(d):
    from graphnet_classifier_amd import native
    _prime(d["w1"].size(0), d["w2"].size(0), d["w3"].size(0))
    return native.readout_forward(d["y"], d["w1"], d["b1"], d["w2"], d["b2"], d["w3"], d["b3"])


def _backward(d, h1, h2, need_dy=True, w1=None):
    from graphnet_classifier_amd import native
    w1 = d["w1"] if w1 is None else w1
    H1, F, H2, C = w1.size(0), w1.size(1), d["w2"].size(0), d["w3"].size(0)
    _prime(F, H1 * F, H1, H2 * H1, H2, C * H2, C)
    return native.readout_backward(d["g"], d["y"], w1, d["w2"], d["w3"], h1, h2, need_dy=need_dy)


def _hold(r, got: dict, what: str):
    """Print every figure, then hold every output of ``got`` to its bar, shape and dtype."""
    errs = {k: (R.max_err(v.cpu(), r["ref"][k]), r["bar"][k]) for k, v in got.items()}
    print(what + ": " + ", ".join(f"{k} {e:.2e}/{b:.2e}" for k, (e, b) in errs.items()))
    for k, v in got.items():
        assert v.shape == r["ref"][k].shape and v.dtype == torch.float32 and v.is_contiguous(), k
    assert all(e <= b for e, b in errs.values()), errs  # a NaN the kernel left is not <= anything


def _run(d, r, what):
    logits, h1, h2 = _forward(d)
    _hold(r, {"logits": logits, "h1": h1, "h2": h2}, what + " forward")
    grads = _backward(d, h1, h2)
    _hold(r, dict(zip(R.GRADS, grads)), what + " backward")
    return (logits, h1, h2) + tuple(grads)


# ------------------------------------------------------------------------------------------------ every shape against float64
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.case_id)
def test_every_shape_matches_float64_and_repeats_bit_for_bit(shape):
    d, r = _dev(R.build(shape)), R.reference_of(shape)
    first = _run(d, r, R.case_id(shape))
    second = _run(d, r, R.case_id(shape) + " again")
    for name, a, b in zip(R.OUTPUTS + R.GRADS, first, second):
        assert torch.equal(a, b), name  # the source documents a fixed summation order


# ------------------------------------------------------------------------------------------------ path selection by layout
def _strided(t, ld, offset=0):
    """The values of the 2-D ``t`` as a view with row stride ``ld`` that starts ``offset`` elements into a NaN-filled buffer."""
    rows, cols = t.shape
    buf = torch.full((offset + rows * ld + 8,), NAN, device=t.device)
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    return view


def _shifted(t):
    """``t`` as a view that starts one element (4 bytes) into a larger buffer: not 16-byte aligned."""
    buf = torch.full((t.numel() + 8,), NAN, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("layout", ["vector_ld_wider", "vector_column_slice", "scalar_ld_odd", "scalar_misaligned", "scalar_y_misaligned"])
@pytest.mark.parametrize("strided_w23", [False, True], ids=["w23_dense", "w23_strided"])
def test_each_fc1_path_by_layout_matches_float64(layout, strided_w23):
    """The same values laid out so that the kernel takes the float4 path (ld1 > F) or the scalar path (ld1 % 4 != 0, w1 or y
    off 16-byte alignment); each against float64, since the summation orders differ."""
    from graphnet_classifier_amd import native
    F = LAYOUT_SHAPE[0]
    d, r = _dev(R.build(LAYOUT_SHAPE)), R.reference_of(LAYOUT_SHAPE)
    if layout == "vector_ld_wider":
        d["w1"] = _strided(d["w1"], F + 12)
    elif layout == "vector_column_slice":
        d["w1"] = _strided(d["w1"], F + 12, offset=4)  # columns 4 .. 4 + F of a wider matrix: still 16-byte aligned
    elif layout == "scalar_ld_odd":
        d["w1"] = _strided(d["w1"], F + 3)
    elif layout == "scalar_misaligned":
        d["w1"], d["y"] = _shifted(d["w1"]), _shifted(d["y"])
    else:
        d["y"] = _shifted(d["y"])
    if strided_w23:
        d["w2"], d["w3"] = _strided(d["w2"], d["w2"].size(1) + 5), _strided(d["w3"], d["w3"].size(1) + 1, offset=3)
    w1 = native._rowmajor(d["w1"])
    assert w1.data_ptr() == d["w1"].data_ptr() and d["y"].is_contiguous()  # the wrapper passes the layout on, no copy
    vector = native._ld(w1) % 4 == 0 and (w1.data_ptr() | d["y"].data_ptr()) % 16 == 0
    assert vector == layout.startswith("vector") and F % 4 == 0
    if strided_w23:
        assert native._ld(native._rowmajor(d["w2"])) == 133 and native._ld(native._rowmajor(d["w3"])) == 33
    _run(d, r, f"{layout} {'strided' if strided_w23 else 'dense'} w2/w3")


# ------------------------------------------------------------------------------------------------ biases, need_dy
@pytest.mark.parametrize("keep", list(itertools.product((True, False), repeat=3)), ids=lambda k: "b" + "".join(str(int(v)) for v in k))
def test_each_bias_may_be_absent(keep):
    d, r = _dev(R.without_biases(R.build(R.BIAS_SHAPE), keep)), R.reference_of(R.BIAS_SHAPE, keep)
    assert [d[b] is not None for b in ("b1", "b2", "b3")] == list(keep)
    _run(d, r, "biases " + str(keep))


@pytest.mark.parametrize("shape", [(255, 7, 5, 3), (257, 65, 33, 5), (1028, 128, 32, 2)], ids=R.case_id)
def test_need_dy_false_leaves_the_other_gradients_bit_equal(shape):
    d = _dev(R.build(shape))
    _, h1, h2 = _forward(d)
    full = _backward(d, h1, h2, need_dy=True)
    part = _backward(d, h1, h2, need_dy=False)
    assert part[0] is None and full[0] is not None
    for name, a, b in zip(R.GRADS[1:], full[1:], part[1:]):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ ReLU edges
def test_units_at_zero_minus_zero_and_below_are_off_with_exactly_zero_gradient():
    c = R.relu_edge_case()
    d, r = _dev(c), R.reference(c)
    units = list(R.EDGE_UNITS)
    out = _run(d, r, "relu edges")
    h1, h2 = out[1], out[2]
    dy, dw1, db1 = out[3], out[4], out[5]
    zero = lambda t: torch.equal(t, torch.zeros_like(t))  # noqa: E731
    assert zero(h1[units]) and zero(db1[units]) and zero(dw1[units])
    assert float(db1.abs().max()) > 0 and float(h1.abs().max()) > 0
    # the units' share of dy: with their rows of w1 back to random values (h1 still says "off"), dy must not move by a bit
    w1_live = _dev(R.build(R.BIAS_SHAPE))["w1"]
    assert float(w1_live[units].abs().min()) > 0
    again = _backward(d, h1, h2, w1=w1_live)
    assert torch.equal(again[0], dy) and zero(again[2][units]) and zero(again[1][units])
    # the same through a mask that h2 carries: a unit of fc2 switched off by hand takes no gradient either
    h2_off = h2.clone()
    live = int(torch.nonzero(h2 > 0)[0])
    h2_off[live] = 0.0
    off = _backward(d, h1, h2_off)
    assert float(off[4][live]) == 0.0 and zero(off[3][live]) and zero(off[5][:, live]) and float(out[7][live]) != 0.0


def test_a_nan_input_reaches_every_logit():
    d = _dev(R.build(R.BIAS_SHAPE))
    d["y"] = d["y"].clone()
    d["y"][130] = NAN
    logits, h1, h2 = _forward(d)
    assert torch.isnan(h1).all() and torch.isnan(h2).all() and torch.isnan(logits).all()  # relu_keep_nan: no finite logits from a poisoned input


# ------------------------------------------------------------------------------------------------ ticket counter
def _ticket():
    from graphnet_classifier_amd import native
    return native._readout_tickets[(DEV, torch.cuda.current_stream(torch.device(DEV)).cuda_stream)]


def test_the_ticket_counter_reads_zero_after_a_call():
    for shape in [(1, 1, 1, 1), (257, 65, 33, 5), (2048, 1024, 96, 64)]:
        _forward(_dev(R.build(shape)))
        t = _ticket()
        assert t.dtype == torch.int32 and t.numel() == 1 and int(t.item()) == 0


def test_64_forwards_back_to_back_equal_their_single_calls():
    d = _dev(R.build((1023, 129, 64, 4)))
    ys = [d["y"], torch.flip(d["y"], dims=[0]).contiguous()]
    single = []
    for y in ys:
        single.append(_forward(dict(d, y=y)))
        torch.cuda.synchronize()
    assert not torch.equal(single[0][0], single[1][0])
    from graphnet_classifier_amd import native
    outs = [native.readout_forward(ys[k % 2], d["w1"], d["b1"], d["w2"], d["b2"], d["w3"], d["b3"]) for k in range(64)]  # no sync
    torch.cuda.synchronize()
    for k, out in enumerate(outs):
        for a, b in zip(out, single[k % 2]):
            assert torch.equal(a, b), k
    assert int(_ticket().item()) == 0


def test_a_second_stream_gets_its_own_counter_and_the_same_bits():
    from graphnet_classifier_amd import native
    d = _dev(R.build((257, 65, 33, 5)))
    eager = _forward(d)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    key = (DEV, side.cuda_stream)
    native._readout_tickets.pop(key, None)  # torch hands streams out of a pool: an earlier user of this one may have left its counter
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = _forward(d)
        grads = _backward(d, out[1], out[2])
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert key in native._readout_tickets and native._readout_tickets[key].data_ptr() != _ticket().data_ptr()
    assert int(native._readout_tickets[key].item()) == 0 and int(_ticket().item()) == 0
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    for a, b in zip(grads, _backward(d, eager[1], eager[2])):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ capture
def test_forward_and_backward_replay_from_one_graph():
    from graphnet_classifier_amd import native
    shape = (1028, 128, 32, 2)
    d = _dev(R.build(shape))
    y, g = d["y"].clone(), d["g"].clone()

    def both(y, g):
        logits, h1, h2 = native.readout_forward(y, d["w1"], d["b1"], d["w2"], d["b2"], d["w3"], d["b3"])
        return (logits, h1, h2) + tuple(native.readout_backward(g, y, d["w1"], d["w2"], d["w3"], h1, h2))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both(y, g)  # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = both(y, g)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for k in range(3):
        y.copy_(torch.randn(y.shape, device=DEV, generator=gen))
        g.copy_(torch.randn(g.shape, device=DEV, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        eager = both(y.clone(), g.clone())
        for name, a, b in zip(R.OUTPUTS + R.GRADS, captured, eager):
            assert torch.equal(a, b), (k, name)
    # the last replay against float64 as well (these y are not screened for the kink: the outputs the mask does not touch)
    r = R.reference(dict(R.build(shape), y=y.cpu().double(), g=g.cpu().double()))
    _hold(r, {k: v for k, v in zip(R.OUTPUTS, captured)}, "replay 3")


# ------------------------------------------------------------------------------------------------ limits
@pytest.mark.parametrize("widths", R.OVER_LIMIT, ids=["H1", "H2", "C"])
def test_widths_past_the_limits_raise_and_the_module_takes_the_torch_path(widths):
    from graphnet_classifier_amd import native
    from graphnet_classifier_amd.GNN import LinearClassifier
    F, H1, H2, C = widths
    c = R.over_limit_case(widths)
    d = _dev(c)
    with pytest.raises(RuntimeError):
        native.readout_forward(d["y"], d["w1"], d["b1"], d["w2"], d["b2"], d["w3"], d["b3"])
    torch.cuda.synchronize()
    m = LinearClassifier(in_features=F, classes=C)
    m.fc1, m.fc2, m.fc3 = torch.nn.Linear(F, H1), torch.nn.Linear(H1, H2), torch.nn.Linear(H2, C)
    m = m.to(DEV)
    with torch.no_grad():
        for k, fc in enumerate((m.fc1, m.fc2, m.fc3), 1):
            fc.weight.copy_(d[f"w{k}"])
            fc.bias.copy_(d[f"b{k}"])
    launches = _launches(lambda: m(d["y"]))
    assert "readout_forward" not in launches[1]
    # the torch path sums in an order of its own: held to what fp32 may be off in ANY order (R.any_order_logits_bound)
    err = (launches[0].detach().cpu().double() - R.evaluate(c)["logits"]).abs()
    bound = R.any_order_logits_bound(c)
    print(f"torch path at {widths}: |logits - float64| {float(err.max()):.2e}, bound {float(bound.min()):.2e} .. {float(bound.max()):.2e}")
    assert launches[0].shape == (C,) and bool((err <= bound).all())


def _launches(fn):
    """(fn(), names of the native launches it made)"""
    from graphnet_classifier_amd import native
    timers = native.KernelTimers()
    native.set_kernel_timers(timers)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        native.set_kernel_timers(None)
    return out, set(timers.events)


# ------------------------------------------------------------------------------------------------ autograd surface
@pytest.mark.parametrize("biases", [True, False], ids=["biases", "no_biases"])
@pytest.mark.parametrize("shape", [(257, 65, 33, 5), (1028, 128, 32, 2)], ids=R.case_id)
def test_functional_readout_gradients_match_float64(shape, biases):
    from graphnet_classifier_amd import functional as Fn
    keep = (biases,) * 3
    d, r = _dev(R.without_biases(R.build(shape), keep)), R.reference_of(shape, keep)
    names = ["y", "w1", "w2", "w3"] + (["b1", "b2", "b3"] if biases else [])
    leaves = {k: d[k].clone().requires_grad_(True) for k in names}
    args = [leaves.get(k) for k in R.INPUTS[:7]]
    _prime(shape[1], shape[2], shape[3])
    logits = Fn.readout(*args)
    _prime(shape[0], shape[0] * shape[1], shape[1], shape[1] * shape[2], shape[2], shape[2] * shape[3], shape[3])
    grads = torch.autograd.grad(logits, [leaves[k] for k in names], d["g"])
    of = {"y": "dy", "w1": "dW1", "b1": "db1", "w2": "dW2", "b2": "db2", "w3": "dW3", "b3": "db3"}
    got = {of[k]: g for k, g in zip(names, grads)}
    got["logits"] = logits.detach()
    _hold(r, got, f"functional.readout {R.case_id(shape)} biases={biases}")


def test_an_input_that_needs_no_gradient_gets_none():
    from graphnet_classifier_amd import functional as Fn, native
    d = _dev(R.build((257, 65, 33, 5)))
    w = {k: d[k].clone().requires_grad_(True) for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
    y = d["y"].clone()
    assert not y.requires_grad
    seen = []
    real = native.readout_backward

    def spy(*a, **kw):
        seen.append(kw.get("need_dy", a[7] if len(a) > 7 else True))
        out = real(*a, **kw)
        seen.append(out[0])
        return out
    native.readout_backward = spy
    try:
        Fn.readout(y, *(w[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3"))).backward(d["g"])
    finally:
        native.readout_backward = real
    assert seen == [False, None] and y.grad is None
    r = R.reference_of((257, 65, 33, 5))
    _hold(r, {"dW1": w["w1"].grad, "db1": w["b1"].grad, "dW2": w["w2"].grad, "db2": w["b2"].grad, "dW3": w["w3"].grad,
              "db3": w["b3"].grad}, "no dy")


def test_linear_classifier_uses_the_kernel_for_1d_and_torch_for_2d():
    from graphnet_classifier_amd.GNN import LinearClassifier
    shape = (4096, 128, 32, 2)
    d, r = _dev(R.build(shape)), R.reference_of(shape)
    m = LinearClassifier(in_features=shape[0], classes=shape[3]).to(DEV)
    with torch.no_grad():
        for k, fc in enumerate((m.fc1, m.fc2, m.fc3), 1):
            fc.weight.copy_(d[f"w{k}"])
            fc.bias.copy_(d[f"b{k}"])
    one, names = _launches(lambda: m(d["y"]))
    assert "readout_forward" in names and one.shape == (shape[3],)
    two, names = _launches(lambda: m(d["y"][None]))
    assert "readout_forward" not in names and two.shape == (1, shape[3])
    for out, what in ((one, "kernel"), (two[0], "torch")):
        err = R.max_err(out.detach().cpu(), r["ref"]["logits"])
        print(f"LinearClassifier {what} path: logits {err:.2e}/{r['bar']['logits']:.2e}")
        assert err <= r["bar"]["logits"]
    one.backward(d["g"])
    _hold(r, {"dW1": m.fc1.weight.grad, "db1": m.fc1.bias.grad, "dW2": m.fc2.weight.grad, "db2": m.fc2.bias.grad,
              "dW3": m.fc3.weight.grad, "db3": m.fc3.bias.grad}, "LinearClassifier backward")
