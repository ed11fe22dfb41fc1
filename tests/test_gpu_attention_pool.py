"""GPU: the attention read-out kernels (K19, csrc/attention_pool.hip) through ``native.graph_attention_pool_forward`` /
``functional.graph_attention_pool`` against per-graph float64 torch on the CPU.  The batch is K17's test batch: graphs of 0, 1, 63,
64, 65, R, R + 1, 2R + 37 and 5 rows (R = the plan's ``chunk_rows``) and 40 slack rows behind the last graph, at widths 1, 3, 64 and
130, with two score sets: ``4 randn`` and ``200 randn`` (differences beyond 1000: any form without the max subtraction overflows).

Bounds, with u = 2^-24, alpha the float64 softmax, n the graph's rows and D = max_v (m - s_v) of the graph:
  forward  |got - ref| <= (2n + 2D + 8) u sum_v alpha_v |y[v, c]| + 1e-30   (n additions each in numerator and denominator, the
           rounding of s - m which moves e_v by up to D u relatively, expf within 2 ulp, the product, the division);
  dy       |got - ref| <= (n + 2D + 8) u |ref| + 1e-30;
  ds       |got - ref| <= (2n + 2D + C + 16) u alpha_v sum_c |dout[g, c]| (|y[v, c]| + sum_w alpha_w |y[w, c]|) + 1e-30;
  alpha    within (n + 2D + 8) u relative, |sum alpha - 1| <= (n + 4) u per non-empty graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = (1, 3, 64, 130)
KINDS = ("narrow", "wide")
SLACK = 40
EMPTY, SMALL, LARGE = 0, 4, 7  # positions of the empty graph, the 65-row graph and the 2R + 37 graph
U = 2.0 ** -24


@pytest.fixture(scope="module")
def N():
    from graphnet_classifier_amd import native
    native.load_library()
    return native


@pytest.fixture(scope="module")
def Fn():
    from graphnet_classifier_amd import functional
    return functional


def _reference(y, s, dout, gp):
    """float64 on the CPU, graph by graph: the pooled rows, what the bounds are made of, and autograd's gradients."""
    G, rows, C = gp.numel() - 1, y.size(0), y.size(1)
    ref = {"out": torch.zeros(G, C, dtype=torch.float64), "absw": torch.zeros(G, C, dtype=torch.float64),
           "alpha": torch.zeros(rows, dtype=torch.float64), "D": torch.zeros(G, dtype=torch.float64),
           "n": (gp[1:] - gp[:-1]).double(), "dy": torch.zeros(rows, C, dtype=torch.float64),
           "ds": torch.zeros(rows, dtype=torch.float64), "ds_scale": torch.zeros(rows, dtype=torch.float64),
           "graph_of": torch.full((rows,), -1, dtype=torch.int64)}
    for g in range(G):
        a, b = int(gp[g]), int(gp[g + 1])
        if a == b:
            continue
        yg, sg = y[a:b].double().requires_grad_(True), s[a:b].double().requires_grad_(True)
        alpha = torch.softmax(sg, 0)
        out = alpha @ yg
        (out * dout[g].double()).sum().backward()
        alpha = alpha.detach()
        ref["out"][g], ref["absw"][g] = out.detach(), alpha @ yg.detach().abs()
        ref["alpha"][a:b], ref["D"][g] = alpha, float((sg.detach().max() - sg.detach()).max())
        ref["dy"][a:b], ref["ds"][a:b] = yg.grad, sg.grad
        ref["ds_scale"][a:b] = alpha * ((yg.detach().abs() + ref["absw"][g]) * dout[g].double().abs()).sum(1)
        ref["graph_of"][a:b] = g
    return ref


@pytest.fixture(scope="module")
def batch(N):
    """Sizes, offsets, the inputs (CPU) and their float64 references, computed once and never modified."""
    R = N.graph_pool_plan(1000, 64, 9)["chunk_rows"]
    sizes = [0, 1, 63, 64, 65, R, R + 1, 2 * R + 37, 5]
    gp = torch.tensor([0] + sizes).cumsum(0)
    rows = int(gp[-1]) + SLACK
    gen = torch.Generator().manual_seed(20240917)
    out = {"R": R, "sizes": sizes, "gp": gp, "rows": rows, "inside": int(gp[-1]), "y": {}, "dout": {}, "ref": {}}
    for C in WIDTHS:
        out["y"][C] = torch.randn(rows, C, generator=gen)
    base = torch.randn(rows, generator=gen)
    out["s"] = {"narrow": 4 * base, "wide": 200 * base}
    for C in WIDTHS:
        out["dout"][C] = torch.randn(len(sizes), C, generator=gen)
        for kind in KINDS:
            out["ref"][C, kind] = _reference(out["y"][C], out["s"][kind], out["dout"][C], gp)
    assert float(out["ref"][64, "wide"]["D"].max()) > 1000.0  # exp of such a difference overflows without the max subtraction
    return out


def _forward(N, y, s, gp):
    out, saved = N.graph_attention_pool_forward(y.to(DEV), s.to(DEV), gp.to(DEV))
    torch.cuda.synchronize()
    return out.cpu(), saved.cpu()


def _grads(Fn, y, s, gp, dout, need_dy=True, need_ds=True):
    """(out, dy, ds) through the autograd Function; an unwanted gradient is None."""
    yd, sd = y.to(DEV).requires_grad_(need_dy), s.to(DEV).requires_grad_(need_ds)
    out = Fn.graph_attention_pool(yd, sd, gp.to(DEV))
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), (yd.grad.cpu() if need_dy else None), (sd.grad.cpu() if need_ds else None)


def _plus_zero(t):
    return not t.any() and not torch.signbit(t).any()


def _forward_bound(ref):
    return (2 * ref["n"] + 2 * ref["D"] + 8)[:, None] * U * ref["absw"] + 1e-30


def _backward_errors_and_bounds(ref, dy, ds, inside):
    """(|dy - ref|, its bound, |ds - ref|, its bound) over rows [0, inside); rows of no graph in there have zero references and
    only the absolute slack."""
    C = dy.size(1)
    graph_of = ref["graph_of"][:inside].clamp(min=0)
    n, D = ref["n"][graph_of], ref["D"][graph_of]
    err_dy = (dy[:inside].double() - ref["dy"][:inside]).abs()
    bound_dy = (n + 2 * D + 8)[:, None] * U * ref["dy"][:inside].abs() + 1e-30
    err_ds = (ds[:inside].double() - ref["ds"][:inside]).abs()
    bound_ds = (2 * n + 2 * D + C + 16) * U * ref["ds_scale"][:inside] + 1e-30
    return err_dy, bound_dy, err_ds, bound_ds


def test_the_batch_takes_the_many_graphs_regime_and_the_large_graph_alone_the_split_one(N, batch):
    R, lib = batch["R"], N.load_library()
    for C in WIDTHS:
        assert N.graph_pool_plan(batch["rows"], C, len(batch["sizes"]))["split"] == 0
        assert lib.gnc_graph_attention_pool_workspace_floats(batch["rows"], C, len(batch["sizes"])) == 0
        split = N.graph_pool_plan(2 * R + 37, C, 1)
        assert split["split"] == 1
        assert lib.gnc_graph_attention_pool_workspace_floats(2 * R + 37, C, 1) == split["slots"] * (C + 1)
        assert N.graph_pool_plan(65, C, 1)["split"] == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", WIDTHS)
def test_forward_within_the_bound_and_the_empty_graph_is_plus_zero(N, batch, C, kind):
    ref = batch["ref"][C, kind]
    got, saved = _forward(N, batch["y"][C], batch["s"][kind], batch["gp"])
    assert got.shape == (9, C) and saved.shape == (9, 2)
    err, bound = (got.double() - ref["out"]).abs(), _forward_bound(ref)
    ratio = err[1:] / bound[1:]
    print(f"C = {C}, {kind} scores: worst forward err / bound = {float(ratio.max()):.4f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
    assert _plus_zero(got[EMPTY]) and _plus_zero(saved[EMPTY])
    # what the backward keeps: the graph's maximum, exactly, and the sum of the exponentials
    for g, n in enumerate(batch["sizes"]):
        if n:
            sg = batch["s"][kind][int(batch["gp"][g]):int(batch["gp"][g + 1])]
            assert float(saved[g, 0]) == float(sg.max())
            z = torch.exp(sg.double() - sg.double().max()).sum()
            # n additions, and every e_v within (D + 4) u: the rounding of s - m and expf's 2 ulp
            assert abs(float(saved[g, 1]) - float(z)) <= (n + float(ref["D"][g]) + 4) * U * float(z)


@pytest.mark.parametrize("C", WIDTHS)
def test_a_graph_pooled_alone_gives_the_bits_of_the_batch_and_two_runs_agree(Fn, batch, C):
    y, s, gp, dout = batch["y"][C], batch["s"]["narrow"], batch["gp"], batch["dout"][C]
    got = _grads(Fn, y, s, gp, dout)
    again = _grads(Fn, y, s, gp, dout)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    out, dy, ds = got
    for g in (SMALL, LARGE):  # LARGE alone runs in the split regime, inside the batch in the many-graphs regime
        a, b = int(gp[g]), int(gp[g + 1])
        alone = _grads(Fn, y[a:b].clone(), s[a:b].clone(), torch.tensor([0, b - a]), dout[g:g + 1])
        assert torch.equal(alone[0][0], out[g]), (C, g)
        assert torch.equal(alone[1], dy[a:b]) and torch.equal(alone[2], ds[a:b]), (C, g)
    # and in front of other graphs / behind other rows: position in the batch does not matter either
    a, b = int(gp[LARGE]), int(gp[LARGE + 1])
    moved_y, moved_s = torch.cat([torch.ones(3, C), y[a:b], torch.ones(7, C)]), torch.cat([torch.ones(3), s[a:b], torch.ones(7)])
    other = _grads(Fn, moved_y, moved_s, torch.tensor([0, 3, 3 + b - a, 10 + b - a]), dout[[0, LARGE, 1]])
    assert torch.equal(other[0][1], out[LARGE]) and torch.equal(other[1][3:3 + b - a], dy[a:b]) and torch.equal(other[2][3:3 + b - a], ds[a:b])


def test_graphs_that_do_not_start_at_row_zero_and_rows_in_front_get_zero_gradient(Fn):
    """``graph_ptr[0] > 0``: the rows in front of the first graph belong to no graph, like the slack rows behind the last."""
    gen = torch.Generator().manual_seed(3)
    y, s, dout = torch.randn(50, 8, generator=gen), 4 * torch.randn(50, generator=gen), torch.randn(3, 8, generator=gen)
    gp = torch.tensor([5, 20, 20, 44])
    ref = _reference(y, s, dout, gp)
    out, dy, ds = _grads(Fn, y, s, gp, dout)
    assert bool(((out.double() - ref["out"]).abs() <= _forward_bound(ref)).all()) and _plus_zero(out[1])
    for lo, hi in ((0, 5), (44, 50)):
        assert _plus_zero(dy[lo:hi]) and _plus_zero(ds[lo:hi])
    assert bool(dy[5:44].any()) and bool(ds[5:44].any())
    err_dy, bound_dy, err_ds, bound_ds = _backward_errors_and_bounds(ref, dy, ds, 44)
    assert bool((err_dy[5:] <= bound_dy[5:]).all()) and bool((err_ds[5:] <= bound_ds[5:]).all())


@pytest.mark.parametrize("C", (3, 64))
def test_non_finite_values_stay_inside_their_graph(N, batch, C):
    y, s, gp = batch["y"][C], batch["s"]["narrow"], batch["gp"]
    clean, _ = _forward(N, y, s, gp)
    k = int(gp[SMALL]) + 17
    s_bad = s.clone()
    s_bad[k] = float("nan")
    got, _ = _forward(N, y, s_bad, gp)
    bad = torch.zeros(9, C, dtype=torch.bool)
    bad[SMALL] = True
    assert torch.equal(torch.isnan(got), bad) and torch.equal(got[~bad], clean[~bad])
    col = C - 2
    y_bad = y.clone()
    y_bad[k, col] = float("nan")
    got, _ = _forward(N, y_bad, s, gp)
    bad = torch.zeros(9, C, dtype=torch.bool)
    bad[SMALL, col] = True
    assert torch.equal(torch.isnan(got), bad) and torch.equal(got[~bad], clean[~bad])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", WIDTHS)
def test_backward(Fn, batch, C, kind):
    y, s, gp, dout, ref = batch["y"][C], batch["s"][kind], batch["gp"], batch["dout"][C], batch["ref"][C, kind]
    inside, rows = batch["inside"], batch["rows"]
    out, dy, ds = _grads(Fn, y, s, gp, dout)
    assert dy.shape == (rows, C) and ds.shape == (rows,)
    assert _plus_zero(dy[inside:]) and _plus_zero(ds[inside:])  # slack rows: exact +0.0
    err_dy, bound_dy, err_ds, bound_ds = _backward_errors_and_bounds(ref, dy, ds, inside)
    print(f"C = {C}, {kind} scores: worst dy err / bound = {float((err_dy / bound_dy).max()):.4f}, "
          f"ds err / bound = {float((err_ds / bound_ds).max()):.4f}")
    assert bool(torch.isfinite(dy).all()) and bool(torch.isfinite(ds).all())
    assert bool((err_dy <= bound_dy).all())
    assert bool((err_ds <= bound_ds).all())
    # a call that wants one gradient alone returns the same bits for it
    _, dy_only, none = _grads(Fn, y, s, gp, dout, need_ds=False)
    assert none is None and torch.equal(dy_only, dy)
    _, none, ds_only = _grads(Fn, y, s, gp, dout, need_dy=False)
    assert none is None and torch.equal(ds_only, ds)


@pytest.mark.parametrize("C", (1, 64))
def test_backward_and_weights_beyond_two_passes_of_the_capped_grid(Fn, C):
    """attn_backward_kernel runs at most 8 workgroups per CU, 256 / lanes rows each per trip (C = 1: one lane per row, 256 rows;
    C = 64: 16 lanes, 16 rows); attn_weights_kernel 8 x 256 rows per CU.  Two full passes and 1027 rows more, 300 graphs of
    random sizes and 40 slack rows, against the same float64 reference and bounds as ``test_backward`` / ``test_return_weights``.
    At C = 1 the row count is also two passes and 1027 rows of the weights kernel."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = {1: 1, 64: 16}[C]
    rows = 2 * 8 * cus * (256 // lanes) + 1027
    assert rows > 2 * 8 * cus * (256 // lanes) and (C != 1 or rows > 2 * 8 * cus * 256)
    gen = torch.Generator().manual_seed(40 + C)
    inside = rows - SLACK
    cuts = torch.randperm(inside - 1, generator=gen)[:299].sort().values + 1
    gp = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([inside])])
    y, s, dout = torch.randn(rows, C, generator=gen), 4 * torch.randn(rows, generator=gen), torch.randn(300, C, generator=gen)
    ref = _reference(y, s, dout, gp)
    out, dy, ds = _grads(Fn, y, s, gp, dout)
    assert _plus_zero(dy[inside:]) and _plus_zero(ds[inside:])
    err_dy, bound_dy, err_ds, bound_ds = _backward_errors_and_bounds(ref, dy, ds, inside)
    print(f"C = {C}, {rows} rows: worst dy err / bound = {float((err_dy / bound_dy).max()):.4f}, "
          f"ds err / bound = {float((err_ds / bound_ds).max()):.4f}")
    assert bool((err_dy <= bound_dy).all()) and bool((err_ds <= bound_ds).all())
    _, alpha = Fn.graph_attention_pool(y.to(DEV), s.to(DEV), gp.to(DEV), return_weights=True)
    alpha = alpha.cpu()
    assert _plus_zero(alpha[inside:])
    n, D = ref["n"][ref["graph_of"][:inside]], ref["D"][ref["graph_of"][:inside]]
    err = (alpha[:inside].double() - ref["alpha"][:inside]).abs()
    assert bool((err <= (n + 2 * D + 8) * U * ref["alpha"][:inside] + 2.0 ** -126).all())


@pytest.mark.parametrize("kind", KINDS)
def test_return_weights(Fn, batch, kind):
    C = 3
    y, s, gp, ref = batch["y"][C], batch["s"][kind], batch["gp"], batch["ref"][C, kind]
    yd, sd = y.to(DEV).requires_grad_(True), s.to(DEV).requires_grad_(True)
    out, alpha = Fn.graph_attention_pool(yd, sd, gp.to(DEV), return_weights=True)
    assert out.requires_grad and not alpha.requires_grad and alpha.shape == (batch["rows"],) and alpha.dtype == torch.float32
    assert torch.equal(out.detach(), Fn.graph_attention_pool(yd, sd, gp.to(DEV)).detach())
    alpha = alpha.cpu()
    inside = batch["inside"]
    assert bool((alpha >= 0).all()) and _plus_zero(alpha[inside:])
    graph_of = ref["graph_of"][:inside]
    n, D = ref["n"][graph_of], ref["D"][graph_of]
    err = (alpha[:inside].double() - ref["alpha"][:inside]).abs()
    # (below the smallest normal float32, 2^-126, a weight is denormal or flushed: there the format itself bounds the error)
    assert bool((err <= (n + 2 * D + 8) * U * ref["alpha"][:inside] + 2.0 ** -126).all())
    for g, size in enumerate(batch["sizes"]):
        if size:
            total = float(alpha[int(gp[g]):int(gp[g + 1])].double().sum())
            assert abs(total - 1.0) <= (size + 4) * U, (g, total)


def test_argument_errors(N, Fn):
    y, s = torch.randn(10, 4, device=DEV), torch.randn(10, device=DEV)
    gp = torch.tensor([0, 10], device=DEV)
    with pytest.raises(ValueError):
        Fn.graph_attention_pool(y, s, gp.int())            # int32 graph_ptr
    with pytest.raises(ValueError):
        Fn.graph_attention_pool(y, s[:9], gp)              # scores of the wrong length
    with pytest.raises(ValueError):
        Fn.graph_attention_pool(y, s.cpu(), gp)            # scores on another device
    with pytest.raises(ValueError):
        Fn.graph_attention_pool(y, s.double(), gp)         # scores of the wrong dtype
    with pytest.raises(ValueError):
        N.graph_attention_pool_forward(y, s[:, None], gp)  # scores of the wrong shape
    out = Fn.graph_attention_pool(y, s, gp)
    assert out.shape == (1, 4)
