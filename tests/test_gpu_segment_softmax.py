"""GPU, kernel level: the attention neighbourhood aggregation K21 (csrc/segment_softmax.hip) against the float64 CPU reference and
the error bars of tests/segment_softmax_cases.py, at the smallest shapes that reach each kernel.

Small regime (one lane group per destination): N = 37, E = 211 with destination degrees 0, 1, 3, 4, 5, 9 and a hub of 70 at D in
{3, 8, 64, 128, 256}, scores randn x {1, 3, 8}, with and without ``perm``; D = 3 and a column-offset view of a wider table run
the scalar kernel.  Chunk regime (64 destinations per wave): N = 64 x CUs + 65, so the last chunk holds ONE destination; E = 4 N;
D in {4, 12, 64, 100, 128, 256}: one lane per row, 64 lanes per row and lane groups with idle lanes (12, 100) besides the widths
in use.  The backward also runs at D = 12 and 100, where the idle lanes of a group feed zeros into its xor tree.

Bars (tests/segment_softmax_cases.py): u = 2^-24, c_v = 2 deg_v + 2 dmax_v + 12;
  forward |err| <= c_v u sum_k alpha_k |x_k|;  saved: m bit for bit, Z within (deg + 2 dmax + 8) u Z;
  grad_src |err| <= c_v u |alpha_k g|;  grad_score |err| <= (c_v + D) u alpha_k sum_c |g| (|x_k| + sum_j alpha_j |x_j|);
  alpha within c_v u alpha, and its sums per destination within deg u of 1.
Equal scores inside every destination: the bits of K18's MEAN kernel (which rests on the device's expf(+0.0) being exactly 1).
"""
import pytest
import torch

from tests import segment_softmax_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = C.U


def _csr(index, n):
    from graphnet_classifier_amd.topology import DestinationCSR
    return DestinationCSR(index.to(DEV), n, torch.device(DEV))


def _bits(a, b):
    """Bit equality of two float32 tensors (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _forward(src_dev, scores_dev, csr, n, sorted_rows):
    """(out, saved) through perm, or on rows and scores gathered into sorted order."""
    from graphnet_classifier_amd import native
    if sorted_rows:
        return native.segment_softmax_csr(native.gather_rows(src_dev, csr.perm), scores_dev[csr.perm.long()], csr.rowptr, None, n)
    return native.segment_softmax_csr(src_dev, scores_dev, csr.rowptr, csr.perm, n)


def _within(err, bar, what):
    used = C.fraction(err, bar)
    print(f"{what}: uses {used:.3f} of its bar")
    assert used <= 1.0, what


def _check_forward(src, scores, index, n, sorted_rows, what, b=None):
    csr = _csr(index, n)
    out, saved = _forward(src.to(DEV), scores.to(DEV), csr, n, sorted_rows)
    assert out.shape == (n, src.size(1)) and saved.shape == (n, 2)
    b = b or C.bars(src, scores, index, n)
    r_out, _, r_m, r_z = b["ref"]
    _within((out.cpu().double() - r_out).abs(), b["forward"], what + " forward")
    assert torch.equal(saved[:, 0].cpu().double(), r_m), what  # the maximum is one of its inputs
    _within((saved[:, 1].cpu().double() - r_z).abs(), b["saved_z"], what + " Z")
    empty = (C.degrees(index, n) == 0).to(DEV)
    assert bool(empty.any())
    zero_bits = torch.zeros((), dtype=torch.int32, device=DEV)
    assert bool((out[empty].view(torch.int32) == zero_bits).all()) and bool((saved[empty].view(torch.int32) == zero_bits).all()), what
    return out, saved, csr


@pytest.mark.parametrize("sorted_rows", (False, True), ids=("perm", "sorted"))
@pytest.mark.parametrize("width", C.SMALL_WIDTHS)
def test_small_regime(width, sorted_rows):
    for scale in C.SCALES:
        index, src, scores, _ = C.small_case(width, scale)
        _check_forward(src, scores, index, C.SMALL_N, sorted_rows, f"small D={width} scale={scale}")


def _chunk_case(width):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * cus + 65
    assert n > 64 * cus and n % 64 == 1  # beyond the small-graph threshold; the last chunk holds one destination
    index = C.chunk_index(n)
    index[-3:] = n - 1  # ... which has rows
    return n, index, C.values(index.numel(), width, seed=100 + width), C.scores_for(index.numel(), 3, seed=100 + width)


_CHUNK_BARS = {}  # width -> the float64 reference and bars of the chunk case, computed once for both row orders


@pytest.mark.parametrize("sorted_rows", (False, True), ids=("perm", "sorted"))
@pytest.mark.parametrize("width", C.CHUNK_WIDTHS)
def test_chunk_regime(width, sorted_rows):
    n, index, src, scores = _chunk_case(width)
    if width not in _CHUNK_BARS:
        _CHUNK_BARS[width] = C.bars(src, scores, index, n)
    out, saved, csr = _check_forward(src, scores, index, n, sorted_rows, f"chunk N={n} D={width}", _CHUNK_BARS[width])
    assert int(C.degrees(index, n)[n - 1]) >= 3 and float(saved[n - 1, 1]) >= 1.0


@pytest.mark.parametrize("sorted_rows", (False, True), ids=("perm", "sorted"))
def test_column_offset_view_runs_the_scalar_kernel_with_the_vector_kernels_bits(sorted_rows):
    """ld_src = 72 != D = 64 and a base 4 bytes past a 16-byte boundary: the scalar kernel; an aligned copy: the vector kernel."""
    from graphnet_classifier_amd import native
    index, _, scores, _ = C.small_case(64, 3)
    n = C.SMALL_N
    wide = C.values(C.SMALL_E, 72, seed=5)
    csr = _csr(index, n)
    wide_dev, s_dev, perm = wide.to(DEV), scores.to(DEV), csr.perm
    if sorted_rows:
        wide_dev, s_dev, perm = native.gather_rows(wide_dev, csr.perm), s_dev[csr.perm.long()], None
    view = wide_dev[:, 1:65]
    assert view.stride(0) == 72 and view.data_ptr() % 16 == 4
    out, saved = native.segment_softmax_csr(view, s_dev, csr.rowptr, perm, n)
    out2, saved2 = native.segment_softmax_csr(view.contiguous(), s_dev, csr.rowptr, perm, n)
    assert _bits(out, out2) and _bits(saved, saved2)
    ref_src = wide[:, 1:65].contiguous()
    _within((out.cpu().double() - C.ref_attention(ref_src, scores, index, n)[0]).abs(), C.bars(ref_src, scores, index, n)["forward"],
            "scalar kernel forward")
    # the backward's scalar kernel on the same view, against the vector kernel on the copy
    grad = C.values(n, 64, seed=6).to(DEV)
    dst = csr.col32 if not sorted_rows else csr.col32[csr.perm.long()]
    g_src, g_s = native.segment_softmax_backward(grad, view, s_dev, out, saved, dst)
    g_src2, g_s2 = native.segment_softmax_backward(grad, view.contiguous(), s_dev, out, saved, dst)
    assert _bits(g_src, g_src2)  # alpha g: one product either way
    b = C.bars(ref_src, scores, index, n, grad.cpu())
    want = C.ref_attention_backward(grad.cpu(), ref_src, scores, index, n)[1]
    if sorted_rows:
        want, b["grad_score"] = want[csr.perm.long().cpu()], b["grad_score"][csr.perm.long().cpu()]
    for name, got in (("scalar", g_s), ("vector", g_s2)):
        _within((got.cpu().double() - want).abs(), b["grad_score"], f"{name} kernel grad_score")


@pytest.mark.parametrize("regime", ("small", "chunk"))
def test_equal_scores_give_the_bits_of_the_mean_kernel(regime):
    """Constant 0.0, and one constant per destination (3.25, and a seeded value each): expf(+0.0f) is 1.0f, the fmaf is the plain add,
    Z is (float)deg and the division is K18's."""
    from graphnet_classifier_amd import native
    widths = C.SMALL_WIDTHS if regime == "small" else (64,)
    for width in widths:
        if regime == "small":
            n, index, src = C.SMALL_N, C.small_index(), C.values(C.SMALL_E, width, seed=50 + width)
        else:
            n, index, src, _ = _chunk_case(width)
        csr = _csr(index, n)
        mean = native.segment_reduce_csr(src.to(DEV), csr.rowptr, csr.perm, n, "mean")[0]
        per_node = torch.randn(n, generator=torch.Generator().manual_seed(7)) * 5
        for what, scores in (("0.0", torch.zeros(index.numel())), ("3.25", torch.full((index.numel(),), 3.25)),
                             ("per destination", per_node[index])):
            out, saved = native.segment_softmax_csr(src.to(DEV), scores.to(DEV), csr.rowptr, csr.perm, n)
            assert _bits(out, mean), (regime, width, what)
            assert torch.equal(saved[:, 1].cpu(), C.degrees(index, n).float()), (regime, width, what)  # Z = (float)deg exactly
        # ... and on sorted rows
        s_sorted = native.gather_rows(src.to(DEV), csr.perm)
        out, _ = native.segment_softmax_csr(s_sorted, per_node[index].to(DEV)[csr.perm.long()], csr.rowptr, None, n)
        assert _bits(out, mean) and _bits(out, native.segment_reduce_csr(s_sorted, csr.rowptr, None, n, "mean")[0])


def test_two_runs_batches_and_edge_orders_give_the_same_bits():
    from graphnet_classifier_amd import native
    index, src, scores, _ = C.small_case(64, 3)
    n, e = C.SMALL_N, C.SMALL_E
    csr = _csr(index, n)
    out, saved = native.segment_softmax_csr(src.to(DEV), scores.to(DEV), csr.rowptr, csr.perm, n)
    again = native.segment_softmax_csr(src.to(DEV), scores.to(DEV), csr.rowptr, csr.perm, n)
    assert _bits(out, again[0]) and _bits(saved, again[1])  # two runs
    sorted_out = _forward(src.to(DEV), scores.to(DEV), csr, n, True)
    assert _bits(out, sorted_out[0]) and _bits(saved, sorted_out[1])  # sorted rows or rows behind perm
    # the graph as the middle block of a block-diagonal batch of three
    other = C.small_index(seed=3)
    b_index = torch.cat([other, index + n, other + 2 * n])
    b_src = torch.cat([C.values(e, 64, seed=13), src, C.values(e, 64, seed=14)])
    b_scores = torch.cat([C.scores_for(e, 3, seed=13), scores, C.scores_for(e, 3, seed=14)])
    b_csr = _csr(b_index, 3 * n)
    got = native.segment_softmax_csr(b_src.to(DEV), b_scores.to(DEV), b_csr.rowptr, b_csr.perm, 3 * n)
    assert _bits(got[0][n:2 * n], out) and _bits(got[1][n:2 * n], saved)
    # another edge order that keeps each destination's own order: a stable sort by a relabelling of the destinations
    p = torch.argsort(torch.randperm(n, generator=torch.Generator().manual_seed(15))[index], stable=True)
    assert not torch.equal(p, torch.arange(e))
    p_csr = _csr(index[p], n)
    got = native.segment_softmax_csr(src[p].to(DEV), scores[p].to(DEV), p_csr.rowptr, p_csr.perm, n)
    assert _bits(got[0], out) and _bits(got[1], saved)
    # the backward and the weights: two runs
    grad = C.values(n, 64, seed=16).to(DEV)
    a = native.segment_softmax_backward(grad, src.to(DEV), scores.to(DEV), out, saved, csr.col32)
    b = native.segment_softmax_backward(grad, src.to(DEV), scores.to(DEV), out, saved, csr.col32)
    assert _bits(a[0], b[0]) and _bits(a[1], b[1])


def test_non_finite_scores_stay_inside_their_destination():
    from graphnet_classifier_amd import native
    index, src, scores, _ = C.small_case(8, 1)
    n = C.SMALL_N
    csr = _csr(index, n)
    clean, clean_saved = native.segment_softmax_csr(src.to(DEV), scores.to(DEV), csr.rowptr, csr.perm, n)
    hub = int(C.degrees(index, n).argmax())
    rows = (index == hub).nonzero().flatten()
    # a NaN score poisons its own destination's row, and nothing else
    bad = scores.clone()
    bad[rows[17]] = float("nan")
    out, saved = native.segment_softmax_csr(src.to(DEV), bad.to(DEV), csr.rowptr, csr.perm, n)
    nan_rows = torch.isnan(out).any(1)
    assert int(nan_rows.sum()) == 1 and bool(nan_rows[hub]) and bool(torch.isnan(out[hub]).all()) and bool(torch.isnan(saved[hub, 1]))
    assert float(saved[hub, 0]) == float(scores[rows][torch.arange(70) != 17].max())  # fmaxf dropped the NaN from m
    keep = torch.arange(n) != hub
    assert _bits(out[keep], clean[keep]) and _bits(saved[keep], clean_saved[keep])
    # a -inf score among finite ones contributes exactly nothing: the bits of the case without that row
    low = scores.clone()
    low[rows[17]] = float("-inf")
    out, saved = native.segment_softmax_csr(src.to(DEV), low.to(DEV), csr.rowptr, csr.perm, n)
    sel = torch.arange(C.SMALL_E) != rows[17]
    less = _csr(index[sel], n)
    want, want_saved = native.segment_softmax_csr(src[sel].to(DEV), scores[sel].to(DEV), less.rowptr, less.perm, n)
    assert _bits(out, want) and _bits(saved, want_saved) and bool(torch.isfinite(out).all())
    alpha = native.segment_softmax_weights(low.to(DEV), saved, csr.col32)
    assert float(alpha[rows[17]]) == 0.0 and not bool(torch.signbit(alpha[rows[17]]))


@pytest.mark.parametrize("width", C.BACKWARD_WIDTHS)
def test_backward_and_weights(width):
    """Through autograd (``functional.segment_softmax_csr``) with ``perm`` and on sorted rows; the weights kernel."""
    from graphnet_classifier_amd import functional as Fn
    from graphnet_classifier_amd import native
    n = C.SMALL_N
    for scale in C.SCALES:
        index, src, scores, grad = C.small_case(width, scale)
        csr = _csr(index, n)
        want_src, want_score = C.ref_attention_backward(grad, src, scores, index, n)
        b = C.bars(src, scores, index, n, grad)
        s = src.to(DEV).requires_grad_(True)
        t = scores.to(DEV).requires_grad_(True)
        out = Fn.segment_softmax_csr(s, t, csr.rowptr, csr.perm, csr.col32, n)
        out.backward(grad.to(DEV))
        what = f"D={width} scale={scale}"
        assert s.grad.shape == src.shape and t.grad.shape == scores.shape
        _within((s.grad.cpu().double() - want_src).abs(), b["grad_src"], what + " grad_src")
        _within((t.grad.cpu().double() - want_score).abs(), b["grad_score"], what + " grad_score")
        # sorted rows (the model's call): dst_of_row is the sorted destination vector; scores as an [E, 1] column
        order = csr.perm.long()
        s2 = native.gather_rows(src.to(DEV), csr.perm).requires_grad_(True)
        t2 = scores.to(DEV)[order].view(-1, 1).requires_grad_(True)
        out2 = Fn.segment_softmax_csr(s2, t2, csr.rowptr, None, csr.col32[order], n)
        out2.backward(grad.to(DEV))
        assert _bits(out2, out) and t2.grad.shape == (C.SMALL_E, 1)
        assert _bits(s2.grad, s.grad[order]) and _bits(t2.grad.view(-1), t.grad[order])
        # the weights: within c_v u alpha of the reference, summing to 1 within deg u per destination
        _, r_alpha, _, _ = C.ref_attention(src, scores, index, n)
        _, saved = native.segment_softmax_csr(src.to(DEV), scores.to(DEV), csr.rowptr, csr.perm, n)
        alpha = native.segment_softmax_weights(scores.to(DEV), saved, csr.col32)
        assert alpha.shape == (C.SMALL_E,)
        _within((alpha.cpu().double() - r_alpha).abs(), b["alpha"], what + " alpha")
        deg = C.degrees(index, n).double()
        sums = torch.zeros(n, dtype=torch.float64).index_add_(0, index, alpha.cpu().double())
        dev1 = (sums - 1).abs()[deg > 0]
        print(f"{what}: |sum alpha - 1| at most {float((dev1 / (deg[deg > 0] * U)).max()):.3f} deg u")
        assert bool((dev1 <= deg[deg > 0] * U).all()) and bool((sums[deg == 0] == 0).all())
    with pytest.raises(ValueError, match="dst_of_row"):
        Fn.segment_softmax_csr(s, t, csr.rowptr, csr.perm, None, n)


def test_scatter_attention_operator():
    from graphnet_classifier_amd import native
    from graphnet_classifier_amd.GNN import scatter_attention, scatter_mean
    index, src, scores, grad = C.small_case(8, 3)
    n = C.SMALL_N
    assert index.dtype == torch.int64 and not bool((index[1:] >= index[:-1]).all())  # unsorted
    csr = _csr(index, n)
    want, _ = native.segment_softmax_csr(src.to(DEV), scores.to(DEV), csr.rowptr, csr.perm, n)
    out = scatter_attention(src.to(DEV), scores.to(DEV), index.to(DEV), dim_size=n)
    assert _bits(out, want)
    # a dim_size beyond the largest id: the extra destinations are empty, exact +0.0
    big = scatter_attention(src.to(DEV), scores.to(DEV), index.to(DEV), dim_size=n + 5)
    assert big.shape == (n + 5, 8) and _bits(big[:n], want) and _bits(big[n:], torch.zeros(5, 8, device=DEV))
    # dim_size=None (one sync), a 1-D src, an [E, 1] score column, CPU tensors in and out
    last = int(index.max()) + 1
    one = scatter_attention(src[:, 0], scores.view(-1, 1), index)
    assert one.shape == (last, 1) and not one.is_cuda and _bits(one, want[:last, :1].cpu())
    assert _bits(scatter_attention(src.to(DEV), torch.zeros(C.SMALL_E), index.to(DEV), dim_size=n),
                 scatter_mean(src.to(DEV), index.to(DEV), dim_size=n))
    with pytest.raises(NotImplementedError):
        scatter_attention(src.to(DEV), scores.to(DEV), index.to(DEV), dim=1)
    with pytest.raises(ValueError):
        scatter_attention(src.to(DEV), scores[:-1].to(DEV), index.to(DEV), dim_size=n)
    # differentiable in src and scores
    s, t = src.to(DEV).requires_grad_(True), scores.to(DEV).requires_grad_(True)
    scatter_attention(s, t, index.to(DEV), dim_size=n).backward(grad.to(DEV))
    want_src, want_score = C.ref_attention_backward(grad, src, scores, index, n)
    b = C.bars(src, scores, index, n, grad)
    _within((s.grad.cpu().double() - want_src).abs(), b["grad_src"], "operator grad_src")
    _within((t.grad.cpu().double() - want_score).abs(), b["grad_score"], "operator grad_score")
