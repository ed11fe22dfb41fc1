"""GPU: the global pooling read-out kernels (K17, csrc/pool_readout.hip) through ``native.graph_pool_forward`` /
``functional.graph_pool`` against per-graph float64 torch on the CPU.  One batch: graphs of 0, 1, 63, 64, 65, R, R + 1, 2R + 37 and
5 rows (R = the plan's ``chunk_rows``) and 40 slack rows behind the last graph, at widths 1, 3, 64 and 130."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = (1, 3, 64, 130)
SLACK = 40
EMPTY, SMALL, LARGE = 0, 4, 7  # positions of the empty graph, the 65-row graph and the 2R + 37 graph


@pytest.fixture(scope="module")
def N():
    from graphnet_classifier_amd import native
    native.load_library()
    return native


@pytest.fixture(scope="module")
def Fn():
    from graphnet_classifier_amd import functional
    return functional


@pytest.fixture(scope="module")
def batch(N):
    """Sizes, offsets and per width: the input (CPU) and its float64 reference, computed once and never modified."""
    R = N.graph_pool_plan(1000, 64, 9)["chunk_rows"]
    sizes = [0, 1, 63, 64, 65, R, R + 1, 2 * R + 37, 5]
    gp = torch.tensor([0] + sizes).cumsum(0)
    rows = int(gp[-1]) + SLACK
    out = {"R": R, "sizes": sizes, "gp": gp, "rows": rows, "y": {}, "ref": {}}
    gen = torch.Generator().manual_seed(20240917)
    for C in WIDTHS:
        y = torch.randn(rows, C, generator=gen)
        ref = {"sum": torch.zeros(len(sizes), C, dtype=torch.float64), "abs": torch.zeros(len(sizes), C, dtype=torch.float64),
               "max": torch.zeros(len(sizes), C), "argmax": torch.full((len(sizes), C), -1, dtype=torch.int64)}
        for g, n in enumerate(sizes):
            a, b = int(gp[g]), int(gp[g + 1])
            if n:
                ref["sum"][g] = y[a:b].double().sum(0)
                ref["abs"][g] = y[a:b].double().abs().sum(0)
                ref["max"][g] = y[a:b].max(0).values
                ref["argmax"][g] = y[a:b].argmax(0) + a
        out["y"][C], out["ref"][C] = y, ref
    return out


def _forward(N, y, gp, modes):
    out, argmax = N.graph_pool_forward(y.to(DEV), gp.to(DEV), modes)
    torch.cuda.synchronize()
    return out.cpu(), (argmax.cpu() if argmax is not None else None)


def test_the_batch_takes_the_many_graphs_regime_and_the_large_graph_alone_the_split_one(N, batch):
    R = batch["R"]
    for C in WIDTHS:
        assert N.graph_pool_plan(batch["rows"], C, len(batch["sizes"]))["split"] == 0
        assert N.graph_pool_plan(2 * R + 37, C, 1)["split"] == 1
        assert N.graph_pool_plan(65, C, 1)["split"] == 0


@pytest.mark.parametrize("C", WIDTHS)
def test_max_is_bit_equal_and_argmax_is_the_row(N, batch, C):
    got, argmax = _forward(N, batch["y"][C], batch["gp"], N.POOL_MAX)
    ref = batch["ref"][C]
    assert got.shape == (9, C) and argmax.shape == (9, C) and argmax.dtype == torch.int32
    assert torch.equal(got, ref["max"])  # randn: tie-free
    assert torch.equal(argmax.long(), ref["argmax"])


@pytest.mark.parametrize("C", WIDTHS)
def test_sum_and_mean_within_the_worst_case_bound_of_fp32_summation(N, batch, C):
    """|got - ref64| <= (n + 2) 2^-24 sum_r |y[r, c]|: n - 1 additions in any order, the addition onto +0.0 and the final rounding;
    the mean's bound is that over n (the division is correctly rounded: one more half ulp, inside the + 2)."""
    ref = batch["ref"][C]
    n = torch.tensor(batch["sizes"], dtype=torch.float64)[:, None]
    got_sum, _ = _forward(N, batch["y"][C], batch["gp"], N.POOL_SUM)
    got_mean, _ = _forward(N, batch["y"][C], batch["gp"], N.POOL_MEAN)
    bound = (n + 2) * 2.0 ** -24 * ref["abs"]
    err_sum = (got_sum.double() - ref["sum"]).abs()
    err_mean = (got_mean.double() - ref["sum"] / n.clamp(min=1)).abs()
    print(f"C = {C}: worst sum err / bound = {float((err_sum / bound.clamp(min=1e-300)).max()):.3f}, "
          f"mean = {float((err_mean / (bound / n.clamp(min=1)).clamp(min=1e-300)).max()):.3f}")
    assert bool((err_sum <= bound).all())
    assert bool((err_mean <= bound / n.clamp(min=1)).all())


@pytest.mark.parametrize("C", WIDTHS)
def test_empty_graph_is_exact_zero_and_hybrid_is_the_three_modes_side_by_side(N, batch, C):
    y, gp = batch["y"][C], batch["gp"]
    singles = {}
    for name in ("mean", "max", "sum"):
        singles[name], argmax = _forward(N, y, gp, N.POOL_MODES[name])
        row = singles[name][EMPTY]
        assert not row.any() and not torch.signbit(row).any()  # +0.0
        if argmax is not None:
            assert bool((argmax[EMPTY] == -1).all()) and bool((argmax[1:] >= 0).all())
    hybrid, argmax = _forward(N, y, gp, N.POOL_MODES["hybrid"])
    assert hybrid.shape == (9, 3 * C)
    assert torch.equal(hybrid, torch.cat([singles["mean"], singles["max"], singles["sum"]], dim=1))
    assert not hybrid[EMPTY].any() and not torch.signbit(hybrid[EMPTY]).any() and bool((argmax[EMPTY] == -1).all())


@pytest.mark.parametrize("C", WIDTHS)
def test_a_graph_pooled_alone_gives_the_bits_of_the_batch_and_two_runs_agree(N, batch, C):
    y, gp = batch["y"][C], batch["gp"]
    modes = N.POOL_MODES["hybrid"]
    got, argmax = _forward(N, y, gp, modes)
    again, argmax2 = _forward(N, y, gp, modes)
    assert torch.equal(got, again) and torch.equal(argmax, argmax2)
    for g in (SMALL, LARGE):  # LARGE alone runs in the split regime, inside the batch in the many-graphs regime
        a, b = int(gp[g]), int(gp[g + 1])
        alone, alone_arg = _forward(N, y[a:b].clone(), torch.tensor([0, b - a]), modes)
        assert torch.equal(alone[0], got[g]), (C, g)
        assert torch.equal(alone_arg[0] + a, argmax[g])
    # and in front of other graphs / behind other rows: position in the batch does not matter either
    a, b = int(gp[LARGE]), int(gp[LARGE + 1])
    moved = torch.cat([torch.ones(3, C), y[a:b], torch.ones(7, C)])
    other, _ = _forward(N, moved, torch.tensor([0, 3, 3 + b - a, 10 + b - a]), modes)
    assert torch.equal(other[1], got[LARGE])


@pytest.mark.parametrize("C", (3, 64))
def test_ties_go_to_the_lowest_row(N, Fn, batch, C):
    """Small integer values, signed zeros among them: ties are certain.  The expected row is the lowest that holds the maximum;
    checked where it matters, in the backward: dmax lands on exactly that row, exact zeros elsewhere."""
    gp, rows, sizes = batch["gp"], batch["rows"], batch["sizes"]
    gen = torch.Generator().manual_seed(7)
    y = torch.randint(-2, 3, (rows, C), generator=gen).float()
    y[y == 0] = torch.where(torch.rand(int((y == 0).sum()), generator=gen) < 0.5, 0.0, -0.0)
    dmax = torch.randn(len(sizes), C, generator=gen)
    want = torch.zeros(rows, C)
    for g, n in enumerate(sizes):
        a, b = int(gp[g]), int(gp[g + 1])
        for c in range(C if n else 0):
            col = y[a:b, c]
            first = int((col == col.max()).nonzero()[0])  # -0.0 == +0.0
            want[a + first, c] = dmax[g, c]
    yd = y.to(DEV).requires_grad_(True)
    out = Fn.graph_pool(yd, gp.to(DEV), "max")
    out.backward(dmax.to(DEV))
    assert torch.equal(yd.grad.cpu(), want)
    assert torch.equal(out.detach().cpu()[1:], torch.stack([y[int(gp[g]):int(gp[g + 1])].max(0).values for g in range(1, 9)]))


@pytest.mark.parametrize("C", (3, 64))
def test_nan_poisons_its_column_only(N, Fn, batch, C):
    gp, sizes = batch["gp"], batch["sizes"]
    y = batch["y"][C].clone()
    g, col = LARGE, C - 2
    k = int(gp[g]) + batch["R"] + 11  # in the graph's second chunk
    y[k, col] = float("nan")
    y[k + 40, col] = float("nan")     # a later NaN: the FIRST one is the argmax
    got, argmax = _forward(N, y, gp, N.POOL_MODES["hybrid"])
    clean, clean_arg = _forward(N, batch["y"][C], gp, N.POOL_MODES["hybrid"])
    bad = torch.zeros(len(sizes), 3 * C, dtype=torch.bool)
    bad[g, [col, C + col, 2 * C + col]] = True
    assert torch.equal(torch.isnan(got), bad)
    assert torch.equal(got[~bad], clean[~bad])
    assert int(argmax[g, col]) == k
    keep = torch.ones_like(argmax, dtype=torch.bool)
    keep[g, col] = False
    assert torch.equal(argmax[keep], clean_arg[keep])
    yd = y.to(DEV).requires_grad_(True)
    Fn.graph_pool(yd, gp.to(DEV), "max").backward(torch.ones(len(sizes), C, device=DEV))
    dy = yd.grad.cpu()
    assert float(dy[k, col]) == 1.0 and float(dy[:, col].sum()) == float(sum(1 for n in sizes if n))


@pytest.mark.parametrize("C", WIDTHS)
def test_backward(N, Fn, batch, C):
    gp, rows, sizes = batch["gp"], batch["rows"], batch["sizes"]
    y = batch["y"][C]
    G = len(sizes)
    gen = torch.Generator().manual_seed(11 + C)
    grad = {name: torch.randn(G, C, generator=gen) for name in ("mean", "max", "sum")}
    graph_of = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))  # rows inside the graphs
    inside = int(gp[-1])
    n_of = torch.tensor(sizes, dtype=torch.float64)[graph_of][:, None]
    hit = torch.zeros(inside, C, dtype=torch.bool)
    ref_arg = batch["ref"][C]["argmax"]
    for g, n in enumerate(sizes):
        if n:
            hit[ref_arg[g], torch.arange(C)] = True
    term = {"sum": grad["sum"].double()[graph_of], "mean": grad["mean"].double()[graph_of] / n_of,
            "max": torch.where(hit, grad["max"].double()[graph_of], torch.zeros((), dtype=torch.float64))}

    def run(mode, g_out):
        yd = y.to(DEV).requires_grad_(True)
        Fn.graph_pool(yd, gp.to(DEV), mode).backward(g_out.to(DEV))
        dy = yd.grad.cpu()
        assert dy.shape == (rows, C)
        assert not dy[inside:].any() and not torch.signbit(dy[inside:]).any()  # rows behind graph_ptr[-1]: exact +0.0
        return dy[:inside]

    assert torch.equal(run("sum", grad["sum"]), grad["sum"][graph_of])                       # bit for bit
    assert torch.equal(run("max", grad["max"]).double(), term["max"])                        # exact
    dmean = run("mean", grad["mean"]).double()
    assert bool(((dmean - term["mean"]).abs() <= 2.0 ** -23 * term["mean"].abs()).all())
    dhyb = run("hybrid", torch.cat([grad["mean"], grad["max"], grad["sum"]], dim=1)).double()
    total = term["sum"] + term["mean"] + term["max"]
    bound = 3 * 2.0 ** -23 * (term["sum"].abs() + term["mean"].abs() + term["max"].abs())
    assert bool(((dhyb - total).abs() <= bound).all())


@pytest.mark.parametrize("C", (3, 64))
def test_backward_beyond_two_passes_of_the_capped_grid(N, Fn, C):
    """pool_backward_kernel runs at most 8 workgroups of 256 threads per CU, one item (4 columns of a row at C % 4 == 0, else one)
    per thread and trip: two full passes and 1027 items more, over 300 graphs of random sizes and 40 slack rows.  sum: bit for
    bit; mean: one division, 2^-23 relative; max: exact, at the reference's (tie-free) argmax."""
    from tests import grid_pass_cases as G
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_row = C // 4 if C % 4 == 0 else C
    items = 2 * 8 * cus * 256 + 1027
    rows = -(-items // per_row)
    assert rows * per_row > 2 * 8 * cus * 256
    gen = torch.Generator().manual_seed(5 + C)
    inside = rows - SLACK
    cuts = torch.randperm(inside - 1, generator=gen)[:299].sort().values + 1
    gp = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([inside])])
    sizes = (gp[1:] - gp[:-1])
    graph_of = torch.repeat_interleave(torch.arange(300), sizes)
    y = torch.randn(rows, C, generator=gen)
    grad = {name: torch.randn(300, C, generator=gen) for name in ("mean", "max", "sum")}
    _, ref_arg = G.max_first_row_wins(y[:inside], graph_of, 300)

    def run(mode):
        yd = y.to(DEV).requires_grad_(True)
        Fn.graph_pool(yd, gp.to(DEV), mode).backward(grad[mode].to(DEV))
        dy = yd.grad.cpu()
        assert dy.shape == (rows, C) and not dy[inside:].any() and not torch.signbit(dy[inside:]).any()
        return dy[:inside]

    assert torch.equal(run("sum"), grad["sum"][graph_of])
    hit = ref_arg[graph_of] == torch.arange(inside)[:, None]
    assert torch.equal(run("max"), torch.where(hit, grad["max"][graph_of], torch.zeros(())))
    want = grad["mean"].double()[graph_of] / sizes.double()[graph_of][:, None]
    assert bool(((run("mean").double() - want).abs() <= 2.0 ** -23 * want.abs()).all())


def test_graphs_that_do_not_start_at_row_zero_and_rows_in_front_get_zero_gradient(N, Fn):
    """``graph_ptr[0] > 0``: the rows in front of the first graph belong to no graph, like the slack rows behind the last."""
    y = torch.randn(50, 8, generator=torch.Generator().manual_seed(3))
    gp = torch.tensor([5, 20, 20, 44])
    yd = y.to(DEV).requires_grad_(True)
    out = Fn.graph_pool(yd, gp.to(DEV), "sum")
    out.backward(torch.ones(3, 8, device=DEV))
    want = torch.zeros(50, 8)
    want[5:44] = 1.0
    assert torch.equal(yd.grad.cpu(), want)
    ref = torch.stack([y[5:20].double().sum(0), torch.zeros(8, dtype=torch.float64), y[20:44].double().sum(0)])
    assert float((out.detach().cpu().double() - ref).abs().max()) <= 26 * 2.0 ** -24 * float(y.abs().sum(0).max())
    with pytest.raises(ValueError):
        Fn.graph_pool(yd, gp.to(DEV), "median")
