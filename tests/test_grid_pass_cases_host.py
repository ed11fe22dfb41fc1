"""No GPU: the vectorised references of tests/grid_pass_cases.py (needed at millions of destinations, where the per-destination
loops of segment_reduce_cases / segment_softmax_cases take minutes) against those loops at a small size, and the size formulas."""
import torch

from tests import grid_pass_cases as G
from tests import segment_reduce_cases as R
from tests import segment_softmax_cases as S


def test_vectorised_max_equals_the_per_destination_reference():
    for seed, (n, e, d) in enumerate([(R.SMALL_N, R.SMALL_E, 8), (300, 2000, 5), (50, 40, 3)]):
        index = R.small_index() if e == R.SMALL_E else G.random_index(n, e, seed=seed)
        src = R.values(e, d, seed=seed)
        src[::7] = src[3]  # ties: the lowest row wins
        want, want_arg = R.ref_max(src, index, n)
        got, got_arg = G.max_first_row_wins(src, index, n)
        assert torch.equal(got, want) and torch.equal(got_arg, want_arg)
        assert bool((want_arg == -1).any())


def test_vectorised_attention_bars_equal_the_per_destination_ones():
    for width, scale in ((8, 1), (64, 3), (3, 8)):
        index, src, scores, grad = S.small_case(width, scale)
        want, got = S.bars(src, scores, index, S.SMALL_N, grad), G.attention_bars(src, scores, index, S.SMALL_N, grad)
        for key in ("forward", "saved_z", "alpha", "grad_src", "grad_score"):
            assert torch.allclose(got[key], want[key], rtol=1e-12, atol=0), key
        for key, w in zip(("want_src", "want_score"), S.ref_attention_backward(grad, src, scores, index, S.SMALL_N)):
            assert torch.allclose(got[key], w, rtol=1e-11, atol=1e-12), key  # (the bars are of order 1e-7)
        for g, w in zip(got["ref"], want["ref"]):
            assert torch.allclose(g, w, rtol=1e-12, atol=1e-15)
        assert torch.equal(got["ref"][2], want["ref"][2])  # the maximum is one of the scores


def test_integer_operands_keep_every_sum_exact():
    a, b = G.ints(1000, 5, seed=1), G.ints(1000, 7, seed=2)
    assert set(a.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    c, cs = G.xty_ref(a, b)
    assert torch.equal(c, (a.long().t() @ b.long()).double()) and torch.equal(cs, a.long().sum(0).double())
    assert torch.equal(a.t() @ b, c.float())  # fp32 accumulation of these integers is exact
    index = G.random_index(40, 1000, seed=3)
    assert torch.equal(G.scatter_sum_ref(a, index, 40), torch.zeros(40, 5).index_add_(0, index, a))


def test_size_formulas_at_256_compute_units():
    assert [G.xty_rows(p) for p in (2048, 512, 256)] == [131239, 32935, 16551]
    assert G.colsum_rows(256) == 131159
    assert G.row_pass_stride(256, 64) == 16384 and G.row_pass_rows(256, 64) == 57347
    assert [G.lanes_for(d) for d in (4, 12, 64, 100, 200, 256)] == [1, 4, 16, 32, 64, 64]
