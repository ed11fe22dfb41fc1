"""GPU, kernel level: the weight-gradient products (xty_kernel, xty_wg_kernel, reduce_partials_kernel, colsum_pair_kernel of
csrc/mlp_backward.hip; xty_small_kernel of csrc/xty_small.hip) at row counts where every worker of the persistent grid makes
at least THREE trips through its tile loop: the double-buffered LDS tile set of xty_wg_kernel, the register prefetch of the next
tile with its clamped last index, and the 16-wave instance of the small-batch product.

Row counts come from the device: P = gnc_xty_partials_for(huge, M, K) workers in a full grid, rows = 2 P 32 + 5 x 32 + 7 (two
full passes, five workers on a third trip, a ragged last tile of 7 rows).  Every test asserts that premise before it launches.

Integer cases (tests/grid_pass_cases.py): operands from {-2 .. 2}; every partial sum is an exactly representable integer, so C
and the column sums must have the BITS of the float64 product cast to fp32 - no tolerance.  One N(0, 1) case per kernel instance
checks the rounding against float64 with the bound rows 2^-24 (|A|^T |B|) elementwise, computed from its own operands.
"""
import pytest
import torch

from tests import grid_pass_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HUGE = 1 << 30


@pytest.fixture(scope="module")
def native():
    from graphnet_classifier_amd import native as n
    n.load_library()
    return n


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(a, b):
    """Bit equality of two float32 tensors."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _blocks(native, m, k):
    """The [mm, kk] blocks native.xty cuts an [M, K] product into (one gnc_xty_f32 launch each)."""
    out = []
    for _, mm in native._xty_spans(m, 256 if k > 64 else 128):
        for _, kk in native._xty_spans(k, 256 if mm > 64 else 128):
            out += [(mm1, kk) for _, mm1 in native._xty_spans(mm, 128)] if kk <= 64 and mm > 128 else [(mm, kk)]
    return out


def _rows_with_three_trips(native, m, k):
    """rows = 2 P 32 + 5 x 32 + 7 with P the first-pass worker count of the case; the premise is asserted for every launch."""
    lib = native.load_library()
    blocks = _blocks(native, m, k)
    workers = max(lib.gnc_xty_partials_for(HUGE, mm, kk) for mm, kk in blocks)
    rows = G.xty_rows(workers)
    for mm, kk in blocks:
        p = lib.gnc_xty_partials_for(rows, mm, kk)
        assert p * G.RPW * 2 < rows, f"block {mm} x {kk}: {p} workers make fewer than three trips over {rows} rows"
        assert p == lib.gnc_xty_partials_for(HUGE, mm, kk), "the grid is not at its cap"
        # reduce_partials_kernel: eight lanes per column, 4 partials each per unrolled trip
        assert p >= 3 * 32, f"block {mm} x {kk}: reduce_partials makes fewer than three unrolled trips over {p} partials"
    assert rows % G.RPW == 7
    return rows


def _assert_integer_product(c, cs, a, b, what):
    ref_c, ref_cs = G.xty_ref(a, b)
    bad = (c.cpu().double() != ref_c).nonzero()
    assert _bits(c.cpu(), ref_c.float()), f"{what}: {bad.size(0)} wrong entries of C, first at {bad[:4].tolist()}, " \
                                          f"differences {(c.cpu().double() - ref_c)[tuple(bad[:4].t())].tolist()}"
    assert _bits(cs.cpu(), ref_cs.float()), f"{what}: column sums off by {(cs.cpu().double() - ref_cs).abs().max()}"


# per-wave kernel (a narrow operand), the four workgroup instances, one call that splits into several blocks
XTY_SHAPES = [(64, 64), (64, 3), (128, 64), (16, 40),
              (128, 128), (65, 65), (96, 256), (256, 128), (200, 72), (256, 256), (129, 129),
              (300, 90)]


@pytest.mark.parametrize("m,k", XTY_SHAPES)
def test_xty_three_trips_per_worker_is_exact_on_integers(native, m, k):
    rows = _rows_with_three_trips(native, m, k)
    a, b = G.ints(rows, m, seed=m * 7 + k), G.ints(rows, k, seed=m * 7 + k + 1)
    c, cs = native.xty(a.to(DEV), b.to(DEV))
    _assert_integer_product(c, cs, a, b, f"xty {m} x {k}, {rows} rows")
    c2, cs2 = native.xty(a.to(DEV), b.to(DEV))
    assert _bits(c, c2) and _bits(cs, cs2)


# column slices of wider tables: leading dimension % 4 == 0 at a 16-B offset (vector loader), and % 4 != 0 (scalar loader)
def _slice_of_wider(t, vector, seed):
    """``t`` on the device as a column slice: 4 columns in and ld % 4 == 0 (16-B rows: the vector loader), or 3 columns in
    and ld % 4 == 1 (the scalar loader)."""
    width = t.size(1)
    left = 4 if vector else 3
    right = 4 + (-(left + width + 4) + (0 if vector else 1)) % 4
    view = G.in_wider(t, left, right, seed).to(DEV)[:, left:left + width]
    assert view.stride(0) % 4 == (0 if vector else 1) and (view.data_ptr() % 16 == 0) == vector
    return view


@pytest.mark.parametrize("vector", [True, False], ids=["ld_multiple_of_4", "ld_odd_scalar_loader"])
@pytest.mark.parametrize("m,k", [(128, 64), (129, 129)], ids=["per_wave", "workgroup"])
def test_xty_three_trips_on_column_slices(native, m, k, vector):
    rows = _rows_with_three_trips(native, m, k)
    a, b = G.ints(rows, m, seed=31), G.ints(rows, k, seed=32)
    va, vb = _slice_of_wider(a, vector, seed=33), _slice_of_wider(b, vector, seed=34)
    c, cs = native.xty(va, vb)
    _assert_integer_product(c, cs, a, b, f"xty {m} x {k} on slices, ld {va.stride(0)} / {vb.stride(0)}")


@pytest.mark.parametrize("m,k", [(128, 64), (128, 128), (96, 256), (256, 128), (256, 256)],
                         ids=["per_wave", "wg128x128", "wg128x256", "wg256x128", "wg256x256"])
def test_xty_three_trips_rounding_within_the_recursive_sum_bound(native, m, k):
    rows = _rows_with_three_trips(native, m, k)
    a, b = G.normals(rows, m, seed=m + k), G.normals(rows, k, seed=m + k + 1)
    c, cs = native.xty(a.to(DEV), b.to(DEV))
    ref_c, ref_cs = G.xty_ref(a, b)
    bound_c, bound_cs = G.xty_bounds(a, b)
    used_c = float(((c.cpu().double() - ref_c).abs() / bound_c).max())
    used_cs = float(((cs.cpu().double() - ref_cs).abs() / bound_cs).max())
    print(f"xty {m} x {k}, {rows} rows: err / bound at most {used_c:.3e} (C), {used_cs:.3e} (column sums)")
    assert used_c <= 1.0 and used_cs <= 1.0


@pytest.mark.parametrize("width", [64, 40, 200])
def test_colsum_pair_three_trips_is_exact_on_integers(native, width):
    cus = _cus()
    rows = G.colsum_rows(cus)
    waves = native.load_library().gnc_xty_partials(rows)
    assert waves == 8 * cus and waves * 16 * 2 < rows and rows % 16 == 7
    g, y = G.ints(rows, width, seed=width), G.ints(rows, width, seed=width + 1)
    sg, sgy = native.colsum_pair(g.to(DEV), y.to(DEV))
    assert _bits(sg.cpu(), g.double().sum(0).float())
    assert _bits(sgy.cpu(), (g.double() * y.double()).sum(0).float())


# ------------------------------------------------------------------------------------------------ xty_multi (xty_small.hip)
def _lim(native):
    return native.load_library().gnc_xty_small_max_rows()


@pytest.mark.parametrize("m,k", [(128, 128), (100, 3), (17, 72)])
@pytest.mark.parametrize("where", ["4095", "4096", "4099", "lim", "lim+1"])
def test_xty_multi_split_regimes_and_the_hand_over_are_exact_on_integers(native, m, k, where):
    """4,095 rows: 8 splits; 4,096 / 4,099 / lim: 16 splits (the 1024-thread instance); lim + 1: handed to xty."""
    lim = _lim(native)
    assert lim > 4099 and 4 * (lim + 1) < 2 ** 24
    rows = {"lim": lim, "lim+1": lim + 1}.get(where) or int(where)
    a, b = G.ints(rows, m, seed=rows + m), G.ints(rows, k, seed=rows + k + 1)
    (res,), sums = native.xty_multi([(a.to(DEV), b.to(DEV), None)])
    assert sums == []
    _assert_integer_product(res[0], res[1], a, b, f"xty_multi {m} x {k}, {rows} rows")


def test_xty_multi_mixed_launch_gives_each_job_the_bits_of_its_own_launch(native):
    """One launch of a 16-split, a 4-split and an 8-split product and a strided kind-1 row-sum job (the 1024-thread instance for
    all of them): integer data, so every result equals the float64 reference bit for bit; each job's bits also equal those of
    the job launched alone (the property stated above xty_splits), and an output written into a column block of a wider
    gradient leaves the rest of it untouched."""
    assert _lim(native) >= 4099
    shapes = [(4099, 128, 128), (1000, 100, 3), (2048, 17, 72)]
    from graphnet_classifier_amd.native import GNC_XTY_MAX_JOBS
    assert len(shapes) + 1 <= GNC_XTY_MAX_JOBS  # one launch
    ops = [(G.ints(r, m, seed=r + m), G.ints(r, k, seed=r + k + 1)) for r, m, k in shapes]
    part_wide = G.in_wider(G.ints(4099, 200, seed=77), 4, 4, seed=78)
    part = part_wide.to(DEV)[:, 4:204]
    assert part.stride(0) == 208
    wide = torch.full((100, 11), 7.5, device=DEV)  # the [100, 3] product lands in columns 5..7 of this gradient
    outs = [None, wide[:, 5:8], None]
    res, sums = native.xty_multi([(a.to(DEV), b.to(DEV), o) for (a, b), o in zip(ops, outs)], [part])
    for (c, cs), (a, b), (r, m, k) in zip(res, ops, shapes):
        _assert_integer_product(c, cs, a, b, f"mixed launch, job {m} x {k} of {r} rows")
    assert res[1][0].data_ptr() == wide[:, 5:8].data_ptr()
    keep = torch.ones(11, dtype=torch.bool)
    keep[5:8] = False
    assert bool((wide[:, keep.to(DEV)] == 7.5).all())
    assert _bits(sums[0].cpu(), part_wide[:, 4:204].double().sum(0).float())
    for (c, cs), (a, b) in zip(res, ops):  # alone: a launch of its own wave count
        (alone,), _ = native.xty_multi([(a.to(DEV), b.to(DEV), None)])
        assert _bits(alone[0], c) and _bits(alone[1], cs)
    _, (alone_sum,) = native.xty_multi([], [part])
    assert _bits(alone_sum, sums[0])
