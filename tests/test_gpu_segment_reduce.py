"""GPU, kernel level: the mean / max neighbourhood aggregation K18 (csrc/segment_reduce.hip) against the float64 CPU reference of
tests/segment_reduce_cases.py, at the smallest shapes that reach each kernel.

Small regime (one lane group per destination): N = 37, E = 211 with destination degrees 0, 1, 3, 4, 5, 9 and a hub of 70 - the
unrolled-by-four loop, its tail, the empty row - at D in {3, 8, 64, 128, 256} with and without ``perm``; D = 3 and a
column-offset view of a wider table (``ld_src != D``, unaligned base) run the scalar kernel.  Chunk regime (64 destinations per
wave): N = 64 x CUs + 65, so the last chunk holds ONE destination; E = 4 N; D in {4, 12, 64, 100, 128, 256}: one lane per row,
64 lanes per row and lane groups with idle lanes (12, 100) besides the widths in use.

Bars: max, argmax and the max backward are exact.  Mean: the worst case of fp32 recursive summation, (deg - 1) 2^-24 sum|x| / deg,
plus one rounding of the quotient (2^-24 |mean|) - the form of the K17 bound in tests/test_gpu_pool_readout.py - and bit-equal to
``scatter_sum_csr`` followed by ``div_by_degree``.  Mean backward: 2^-23 relative (one division).
"""
import pytest
import torch

from tests import segment_reduce_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _csr(index, n):
    from graphnet_classifier_amd.topology import DestinationCSR
    return DestinationCSR(index.to(DEV), n, torch.device(DEV))


def _bits(a, b):
    """Bit equality of two float32 tensors (NaN payloads and the sign of zero included)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _sorted_rows(src, csr):
    from graphnet_classifier_amd import native
    return native.gather_rows(src, csr.perm)


def _run(src_dev, csr, n, sorted_rows):
    """(mean, max without argmax, max with argmax, argmax as rows of the ORIGINAL src) through perm or on sorted rows."""
    from graphnet_classifier_amd import native
    if sorted_rows:
        s, perm = _sorted_rows(src_dev, csr), None
    else:
        s, perm = src_dev, csr.perm
    mean, none = native.segment_reduce_csr(s, csr.rowptr, perm, n, "mean")
    mx0, none2 = native.segment_reduce_csr(s, csr.rowptr, perm, n, "max")
    mx1, arg = native.segment_reduce_csr(s, csr.rowptr, perm, n, "max", with_argmax=True)
    assert none is None and none2 is None and arg.dtype == torch.int32
    arg = arg.long()
    if sorted_rows:  # winners are sorted positions k: back to rows of the original table
        arg = torch.where(arg >= 0, csr.perm.long()[arg.clamp(min=0)], arg)
    return mean, mx0, mx1, arg, s, perm


def _check_forward(src, index, n, src_dev, csr, sorted_rows, what):
    from graphnet_classifier_amd import native
    mean, mx0, mx1, arg, s, perm = _run(src_dev, csr, n, sorted_rows)
    r_mean, (r_max, r_arg) = C.ref_mean(src, index, n), C.ref_max(src, index, n)
    deg = C.degrees(index, n).double()[:, None]
    assert _bits(mx0.cpu(), r_max) and _bits(mx1.cpu(), r_max), what
    assert torch.equal(arg.cpu(), r_arg), what
    bound = (deg - 1).clamp(min=0) * U * C.ref_abs_sum(src, index, n) / deg.clamp(min=1) + U * r_mean.abs()
    err = (mean.cpu().double() - r_mean).abs()
    print(f"{what}: mean err {float(err.max()):.3e}, bound at that element {float(bound.flatten()[err.argmax()]):.3e}")
    assert bool((err <= bound).all()), what
    sums = native.scatter_sum_csr(s, csr.rowptr, perm, n)
    assert _bits(native.rows_div_degree_(sums, csr.rowptr), mean), what
    empty = (deg[:, 0] == 0).to(DEV)
    zero_bits = torch.zeros((), dtype=torch.int32, device=DEV)
    for t in (mean, mx0, mx1):
        assert bool((t[empty].view(torch.int32) == zero_bits).all()), what  # exact +0.0
    assert bool((arg[empty] == -1).all()) and bool((arg[~empty] >= 0).all()), what
    return mean, mx1


@pytest.mark.parametrize("sorted_rows", (False, True), ids=("perm", "sorted"))
@pytest.mark.parametrize("width", C.SMALL_WIDTHS)
def test_small_regime(width, sorted_rows):
    index = C.small_index()
    assert sorted(C.degrees(index, C.SMALL_N).tolist()) == sorted(C.SMALL_DEGREES)
    src = C.values(C.SMALL_E, width, seed=width)
    csr = _csr(index, C.SMALL_N)
    _check_forward(src, index, C.SMALL_N, src.to(DEV), csr, sorted_rows, f"small D={width}")


@pytest.mark.parametrize("sorted_rows", (False, True), ids=("perm", "sorted"))
def test_column_offset_view_of_a_wider_table(sorted_rows):
    """ld_src = 72 != D = 64 and a base 4 bytes past a 16-byte boundary: the scalar kernel."""
    from graphnet_classifier_amd import native
    index = C.small_index()
    wide = C.values(C.SMALL_E, 72, seed=5)
    csr = _csr(index, C.SMALL_N)
    wide_dev = wide.to(DEV)
    if sorted_rows:
        wide_dev, perm = native.gather_rows(wide_dev, csr.perm), None
    else:
        perm = csr.perm
    view = wide_dev[:, 1:65]
    assert view.stride(0) == 72 and view.data_ptr() % 16 == 4
    ref_src = wide[:, 1:65].contiguous()
    r_max, r_arg = C.ref_max(ref_src, index, C.SMALL_N)
    mx, arg = native.segment_reduce_csr(view, csr.rowptr, perm, C.SMALL_N, "max", with_argmax=True)
    arg = arg.long()
    if sorted_rows:
        arg = torch.where(arg >= 0, csr.perm.long()[arg.clamp(min=0)], arg)
    assert _bits(mx.cpu(), r_max) and torch.equal(arg.cpu(), r_arg)
    mean, _ = native.segment_reduce_csr(view, csr.rowptr, perm, C.SMALL_N, "mean")
    aligned = ref_src.to(DEV) if not sorted_rows else native.gather_rows(ref_src.to(DEV), csr.perm)
    assert _bits(mean, native.segment_reduce_csr(aligned, csr.rowptr, perm, C.SMALL_N, "mean")[0])  # scalar == vector kernel


@pytest.mark.parametrize("sorted_rows", (False, True), ids=("perm", "sorted"))
@pytest.mark.parametrize("width", C.CHUNK_WIDTHS)
def test_chunk_regime(width, sorted_rows):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * cus + 65
    assert n > 64 * cus and n % 64 == 1  # beyond the small-graph threshold; the last chunk holds one destination
    index = C.chunk_index(n)
    index[-3:] = n - 1  # ... which has rows
    src = C.values(index.numel(), width, seed=100 + width)
    _check_forward(src, index, n, src.to(DEV), _csr(index, n), sorted_rows, f"chunk N={n} D={width}")


def test_ties_signed_zeros_and_the_max_backward():
    """Duplicated rows tie to the lowest row and the gradient goes only there; -0.0 against +0.0 is a tie."""
    from graphnet_classifier_amd import native
    index = C.small_index()
    n, e = C.SMALL_N, C.SMALL_E
    src = C.values(e, 64, seed=9)
    hub = int(C.degrees(index, n).argmax())
    rows = (index == hub).nonzero().flatten()
    src[rows[5]] = src[rows[2]]          # a duplicate of an earlier row of the hub
    src[rows[40]] = src[rows[2]]
    src[rows, 7] = -1.0                  # column 7 of the hub: the maximum is a zero, -0.0 first
    src[rows[3], 7], src[rows[11], 7] = -0.0, 0.0
    csr = _csr(index, n)
    r_max, r_arg = C.ref_max(src, index, n)
    assert int(r_arg[hub, 7]) == int(rows[3]) and not bool((r_arg[hub] == rows[5]).any()) and not bool((r_arg[hub] == rows[40]).any())
    mx, arg = native.segment_reduce_csr(src.to(DEV), csr.rowptr, csr.perm, n, "max", with_argmax=True)
    assert _bits(mx.cpu(), r_max) and torch.equal(arg.long().cpu(), r_arg)
    assert mx[hub, 7].item() == 0.0 and bool(torch.signbit(mx[hub, 7]))
    grad = C.values(n, 64, seed=10)
    got = native.segment_reduce_backward(grad.to(DEV), csr.col32, csr.rowptr, arg, "max")
    want = C.ref_max_backward(grad, index, r_arg)
    assert _bits(got.cpu(), want)
    assert bool((got[rows[5]] == 0).all()) and bool((got[rows[40]] == 0).all())
    assert not bool(torch.signbit(got.cpu()[want == 0]).any())  # exact +0.0 elsewhere


def test_a_nan_poisons_its_own_column_of_its_own_destination():
    from graphnet_classifier_amd import native
    index = C.small_index()
    n = C.SMALL_N
    src = C.values(C.SMALL_E, 8, seed=11)
    clean = src.clone()
    row = int((index == int(C.degrees(index, n).argmax())).nonzero()[17])
    src[row, 3] = float("nan")
    src[int((index == index[row]).nonzero()[30]), 3] = float("nan")  # a second NaN behind it: argmax stays at the first
    csr = _csr(index, n)
    for mode in ("mean", "max"):
        a, arg = native.segment_reduce_csr(src.to(DEV), csr.rowptr, csr.perm, n, mode, with_argmax=mode == "max")
        b, _ = native.segment_reduce_csr(clean.to(DEV), csr.rowptr, csr.perm, n, mode)
        bad = torch.isnan(a)
        assert int(bad.sum()) == 1 and bool(bad[index[row], 3])
        assert _bits(a[~bad], b[~bad])
        if mode == "max":
            assert int(arg[index[row], 3]) == row
            assert torch.equal(arg.long().cpu(), C.ref_max(src, index, n)[1])


def test_two_runs_batches_and_edge_permutations_give_the_same_bits():
    from graphnet_classifier_amd import native
    index, n, e = C.small_index(), C.SMALL_N, C.SMALL_E
    src = C.values(e, 64, seed=12)
    csr = _csr(index, n)
    out = {m: native.segment_reduce_csr(src.to(DEV), csr.rowptr, csr.perm, n, m)[0] for m in ("mean", "max")}
    for m in out:
        assert _bits(out[m], native.segment_reduce_csr(src.to(DEV), csr.rowptr, csr.perm, n, m)[0])  # two runs
    # the graph as the middle block of a block-diagonal batch of three
    other = C.small_index(seed=3)
    b_index = torch.cat([other, index + n, other + 2 * n])
    b_src = torch.cat([C.values(e, 64, seed=13), src, C.values(e, 64, seed=14)])
    b_csr = _csr(b_index, 3 * n)
    for m in out:
        got = native.segment_reduce_csr(b_src.to(DEV), b_csr.rowptr, b_csr.perm, 3 * n, m)[0]
        assert _bits(got[n:2 * n], out[m]), m
    # a permutation of the edge list: the max does not move (the mean's summation order does)
    p = torch.randperm(e, generator=torch.Generator().manual_seed(15))
    p_csr = _csr(index[p], n)
    got, arg = native.segment_reduce_csr(src[p].to(DEV), p_csr.rowptr, p_csr.perm, n, "max", with_argmax=True)
    assert _bits(got, out["max"])
    picked = src[p].to(DEV).gather(0, arg.long().clamp(min=0))  # the winners' rows of the permuted table hold the maxima
    assert _bits(torch.where(arg >= 0, picked, torch.zeros((), device=DEV)), got)


@pytest.mark.parametrize("width", (3, 64))
def test_backward(width):
    """MEAN within 2^-23 relative of float64; MAX exact; through autograd (``segment_*_csr``) and ``div_by_degree``."""
    from graphnet_classifier_amd import functional as Fn
    index, n, e = C.small_index(), C.SMALL_N, C.SMALL_E
    src = C.values(e, width, seed=20 + width)
    grad = C.values(n, width, seed=30 + width)
    csr = _csr(index, n)
    s = src.to(DEV).requires_grad_(True)
    Fn.segment_mean_csr(s, csr.rowptr, csr.perm, csr.col32, n).backward(grad.to(DEV))
    want = C.ref_mean_backward(grad, index, n)
    err = (s.grad.cpu().double() - want).abs()
    assert bool((err <= 2.0 ** -23 * want.abs()).all())
    # the sum followed by div_by_degree: the same gradient bits (the division applied to the gradient, then K2's gather)
    s2 = src.to(DEV).requires_grad_(True)
    mean2 = Fn.div_by_degree(Fn.scatter_sum_csr(s2, csr.rowptr, csr.perm, csr.col32, n), csr.rowptr)
    mean2.backward(grad.to(DEV))
    assert _bits(s2.grad, s.grad)
    s3 = src.to(DEV).requires_grad_(True)
    mx, arg = Fn.segment_max_csr(s3, csr.rowptr, csr.perm, csr.col32, n, return_argmax=True)
    assert not arg.requires_grad
    mx.backward(grad.to(DEV))
    r_arg = C.ref_max(src, index, n)[1]
    assert torch.equal(arg.long().cpu(), r_arg) and _bits(s3.grad.cpu(), C.ref_max_backward(grad, index, r_arg))
    # sorted rows (the model's call): dst_of_row is the sorted destination vector
    from graphnet_classifier_amd import native
    dst_sorted = csr.col32[csr.perm.long()]
    s4 = native.gather_rows(src.to(DEV), csr.perm).requires_grad_(True)
    Fn.segment_max_csr(s4, csr.rowptr, None, dst_sorted, n).backward(grad.to(DEV))
    assert _bits(s4.grad, native.gather_rows(s3.grad, csr.perm))


def test_scatter_mean_and_scatter_max_operators():
    from graphnet_classifier_amd.GNN import scatter_max, scatter_mean, scatter_sum
    index, n = C.small_index(), C.SMALL_N
    src = C.values(C.SMALL_E, 8, seed=40)
    csr = _csr(index, n)
    from graphnet_classifier_amd import native
    mean = scatter_mean(src.to(DEV), index.to(DEV), dim_size=n)
    mx, arg = scatter_max(src.to(DEV), index.to(DEV), dim_size=n)
    assert _bits(mean, native.segment_reduce_csr(native.gather_rows(src.to(DEV), csr.perm), csr.rowptr, None, n, "mean")[0])
    r_max, r_arg = C.ref_max(src, index, n)
    assert _bits(mx.cpu(), r_max) and arg.dtype == torch.int64 and torch.equal(arg.cpu(), r_arg)
    # dim_size=None (one sync), a 1-D src, CPU tensors in and out
    last = int(index.max()) + 1
    m1 = scatter_mean(src[:, 0], index)
    assert m1.shape == (last, 1) and not m1.is_cuda and _bits(m1, mean[:last, :1].cpu())
    x1, a1 = scatter_max(src[:, 0], index)
    assert x1.shape == (last, 1) and _bits(x1, mx[:last, :1].cpu()) and torch.equal(a1, arg[:last, :1].cpu())
    for fn in (scatter_mean, scatter_max):
        with pytest.raises(NotImplementedError):
            fn(src.to(DEV), index.to(DEV), dim=1)
    s = src.to(DEV).requires_grad_(True)
    out, _ = scatter_max(s, index.to(DEV), dim_size=n)
    out.sum().backward()
    assert _bits(s.grad.cpu(), C.ref_max_backward(torch.ones(n, 8), index, r_arg))
    assert _bits(scatter_sum(src.to(DEV), index.to(DEV), dim_size=n), native.scatter_sum_csr(src.to(DEV), csr.rowptr, csr.perm, n))
