"""GPU: the capacity-padded top-K pooling launches (K20, ``gnc_topk_pool_select_padded_f32`` / ``gnc_topk_pool_filter_edges_padded``)
at operator level.  Every integer output is compared for EQUALITY with the layout of tests/topk_pool_padded_cases.py over its whole
length, and its prefix with what the sized launches give on the same inputs; the compacted rows must be the sized launch's bits in
front of N' / E' and exact +0.0 behind, and the backward must not see an upstream gradient row at or behind N' / E'."""
import numpy as np
import pytest
import torch

from tests import topk_pool_cases as K
from tests import topk_pool_padded_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (1, 2, 65, 257, 1025)
EDGES = (0, 1, 257, 1025, 4097)
RATIOS = (1.0, 0.5, 1e-3)
WIDTHS = (3, 64, 65)
BIG = 3.0e30  # a finite upstream gradient that would be seen in any result it reached


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _graph_ptr(rows, G):
    """G graphs over all rows (G = 3: the cuts at rows // 3 and 2 * rows // 3, empty graphs at the smallest sizes)."""
    return np.asarray([0, rows] if G == 1 else [0, rows // 3, 2 * rows // 3, rows], dtype=np.int64)


def _layer(scores, gp, ratio, src, dst, rowptr, status=None):
    """One pooling layer both ways on the device.  The padded result is compared with ``ref_padded`` everywhere, the sized result
    with its prefix.  Returns ``(padded tensors, sized tensors, reference)``."""
    from graphnet_classifier_amd import native
    from graphnet_classifier_amd.topology import GraphTopology
    s, g = _dev(scores), _dev(np.asarray(gp, np.int64))
    edges = [_dev(a) for a in (src, dst, rowptr)]
    ref = P.ref_padded(scores, gp, ratio, src, dst, rowptr)
    n_out, e_out, rows, E = ref["n_out"], ref["e_out"], scores.shape[0], src.shape[0]
    new_id, kept, gp_out, counts = native.topk_pool_select(s, g, ratio, padded=True)
    out = native.topk_pool_filter_edges(*edges, new_id, kept, counts, padded=True)
    got = dict(zip(("src", "dst", "kept_edges", "edge_new_id", "rowptr"), out), new_id=new_id, kept=kept, graph_ptr=gp_out)
    assert counts.tolist() == [n_out, e_out]
    for name, t in got.items():
        a = t.cpu().numpy()
        assert a.shape == ref[name].shape and np.array_equal(a, ref[name]), (name, a[:40], ref[name][:40])
    # the sized launches on the same inputs: the prefixes
    new_id_s, kept_s, gp_s, counts_s = native.topk_pool_select(s, g, ratio)
    out_s = native.topk_pool_filter_edges(*edges, new_id_s, kept_s, counts_s)
    sized = dict(zip(("src", "dst", "kept_edges", "edge_new_id", "rowptr"), out_s), new_id=new_id_s, kept=kept_s, graph_ptr=gp_s)
    assert counts_s.tolist() == [n_out, e_out]
    assert torch.equal(new_id, new_id_s) and torch.equal(gp_out, gp_s) and torch.equal(got["edge_new_id"], sized["edge_new_id"])
    assert torch.equal(kept[:n_out], kept_s[:n_out])
    for name in ("src", "dst", "kept_edges"):
        assert torch.equal(got[name][:e_out], sized[name][:e_out]), name
    every_row_kept_but_an_edge_dropped = n_out == rows and e_out < E  # the S_R == 0 rule moves rowptr'[rows] to E
    upto = n_out if every_row_kept_but_an_edge_dropped else n_out + 1
    assert torch.equal(got["rowptr"][:upto], sized["rowptr"][:upto])
    # what the layout promises, stated on the device result itself: a destination-sorted list over `rows` nodes that ends at E
    d = got["dst"].cpu().numpy()
    assert np.all(np.diff(d) >= 0) and (E == 0 or (d.min() >= 0 and d.max() < rows)) and int(got["rowptr"][-1]) == E
    assert np.array_equal(got["rowptr"].cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(d, minlength=rows))]))
    if n_out < rows and e_out < E:
        assert np.bincount(d[e_out:], minlength=rows).max() <= P.ceil_div(E - e_out, rows - n_out)
    # the padded arrays are a topology as they stand; its lazily built source-sorted view is a stable sort of src'
    status = torch.zeros(2, dtype=torch.int32, device=DEV) if status is None else status
    topo = GraphTopology.from_sorted(got["rowptr"], got["src"], got["dst"], rows, status, False)
    assert topo.num_nodes == rows and topo.num_edges == E
    rp_csc, perm_csc = topo.csc
    sp = got["src"].cpu().numpy()
    assert np.array_equal(perm_csc.cpu().numpy(), np.argsort(sp, kind="stable"))
    assert np.array_equal(rp_csc.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(sp, minlength=rows))]))
    return got, sized, ref


@pytest.mark.parametrize("rows", ROWS)
def test_integer_outputs_at_every_shape(rows):
    """rows x E x ratio x G, a hub destination and self-loops among the edges."""
    for E in EDGES:
        for ratio in RATIOS:
            for G in (1, 3):
                rng = np.random.default_rng(1000 * rows + E + G)
                scores = rng.standard_normal(rows).astype(np.float32)
                src, dst, rowptr = K.sorted_edges(rng, rows, E, hub=True)
                got, _, ref = _layer(scores, _graph_ptr(rows, G), ratio, src, dst, rowptr)
                if ratio == 1.0:  # nothing dropped: no slack, the input's list back
                    assert ref["n_out"] == rows and ref["e_out"] == E and np.array_equal(got["src"].cpu().numpy(), src)


def test_rows_of_no_graph_an_empty_graph_and_special_scores():
    """5 rows in front of the graphs, an empty graph in the middle, 9 rows behind; every score pattern (ties, NaN, infinities)."""
    rng = np.random.default_rng(21)
    gp = np.asarray([5, 135, 135, 400], dtype=np.int64)
    rows = 409
    src, dst, rowptr = K.sorted_edges(rng, rows, 1500, hub=True)
    for name, scores in K.score_patterns(rng, rows).items():
        got, _, ref = _layer(scores, gp, 0.5, src, dst, rowptr)
        assert ref["n_out"] == 65 + 133 and np.all(ref["new_id"][:5] == -1) and np.all(ref["new_id"][400:] == -1), name
        assert int(got["graph_ptr"][-1]) == ref["n_out"] and got["graph_ptr"].tolist()[1] == got["graph_ptr"].tolist()[2]


@pytest.mark.parametrize("ratio", (1.0, 0.5))
def test_endpoints_outside_the_table(ratio):
    """Edges with an endpoint outside [0, rows) are dropped without being an index.  ratio 1 keeps every row, so those edges are the
    only slack there is and S_R == 0: their slots become self-loops of the last row and the offsets still end at E."""
    rng = np.random.default_rng(8)
    rows = 65
    scores = rng.standard_normal(rows).astype(np.float32)
    src, dst, rowptr = K.sorted_edges(rng, rows, 300, hub=True, out_of_range=6)
    got, _, ref = _layer(scores, [0, rows], ratio, src, dst, rowptr)
    E = src.shape[0]
    assert ref["e_out"] < E
    if ratio == 1.0:
        assert ref["n_out"] == rows and bool((got["dst"][ref["e_out"]:] == rows - 1).all()) and bool((got["src"][ref["e_out"]:] == rows - 1).all())
    assert int(got["rowptr"][-1]) == E and int(got["src"].max()) < rows and int(got["src"].min()) >= 0


def _positive_zero(t):
    """Every element is +0.0, sign bit included."""
    return not bool(t.contiguous().view(torch.int32).ne(0).any())


@pytest.mark.parametrize("C,strided", [(C, False) for C in WIDTHS] + [(64, True), (65, True)])
def test_rows_forward_and_backward(C, strided):
    """Node rows (gated) and edge rows (no gate) through the row launches with n_out = rows / E: the sized launch's bits in front,
    +0.0 behind; upstream gradient rows at or behind N' / E' hold large finite values and must reach nothing.  ``strided``: every
    table has a leading dimension above C, NaN between the rows."""
    from graphnet_classifier_amd import native
    rng = np.random.default_rng(C)
    rows, gp = 1031, [3, 400, 400, 1029]
    scores = (2.0 * rng.standard_normal(rows)).astype(np.float32)
    src, dst, rowptr = K.sorted_edges(rng, rows, 2500, hub=True)
    got, sized, ref = _layer(scores, gp, 0.5, src, dst, rowptr)
    n_out, e_out, E = ref["n_out"], ref["e_out"], src.shape[0]
    assert 0 < n_out < rows and 0 < e_out < E
    ld = C + (4 if C % 4 == 0 else 3) if strided else C
    s = _dev(scores)

    def table(n, fill=None):
        full = torch.from_numpy(rng.standard_normal((n, ld)).astype(np.float32)).to(DEV) if fill is None else torch.full((n, ld), fill, device=DEV)
        return full, full[:, :C]

    for index, index_sized, ids, n_in, n_kept, gate in ((got["kept"], sized["kept"][:n_out], got["new_id"], rows, n_out, s),
                                                        (got["kept_edges"], sized["kept_edges"][:e_out], got["edge_new_id"], E, e_out, None)):
        _, x = table(n_in)
        out_full, out = table(n_in, float("nan"))
        native.topk_pool_rows_forward(x, index, gate, out=out)
        want = native.topk_pool_rows_forward(x, index_sized, gate)
        assert torch.equal(out[:n_kept], want) and _positive_zero(out[n_kept:])
        assert not strided or bool(torch.isnan(out_full[:, C:]).all())
        # backward: the padded upstream gradient = the sized one in front, BIG behind
        _, grad = table(n_in, BIG)
        grad[:n_kept] = torch.from_numpy(rng.standard_normal((n_kept, C)).astype(np.float32)).to(DEV)
        dx, ds = native.topk_pool_rows_backward(grad, ids, x if gate is not None else None, gate)
        dx_s, ds_s = native.topk_pool_rows_backward(grad[:n_kept], ids, x if gate is not None else None, gate)
        assert torch.equal(dx, dx_s) and bool(torch.isfinite(dx).all()) and float(dx.abs().max()) < 1e3
        if gate is not None:
            assert torch.equal(ds, ds_s) and bool(torch.isfinite(ds).all())
        else:
            assert ds is None and ds_s is None


def _pool_twice(padded, x, topo, e, gp, scores1, scores2_of):
    """Two pooling layers in a row through ``functional.topk_pool``; ``scores2_of(n)``: the second layer's scores for n rows."""
    from graphnet_classifier_amd import functional as Fn
    x1, e1, topo1, gp1, kept1 = Fn.topk_pool(x, scores1, topo, gp, 0.5, e, padded=padded)
    x2, e2, topo2, gp2, kept2 = Fn.topk_pool(x1, scores2_of(x1.size(0)), topo1, gp1, 0.5, e1, padded=padded)
    return (x1, e1, topo1, gp1, kept1), (x2, e2, topo2, gp2, kept2)


def test_functional_padded_layer_twice_against_the_sized_layers():
    """``functional.topk_pool(padded=True)`` twice in a row on a batch of three graphs with rows of no graph around them, against the
    sized layers on the same inputs: outputs, composed kept set and the gradients of x, the scores and the edge rows.  The second
    layer sees the first one's slack rows as rows of no graph (with tempting scores) and must erase them and their self-loops again."""
    from graphnet_classifier_amd.topology import GraphTopology
    rng = np.random.default_rng(4)
    rows, C, De = 521, 8, 5
    gp = torch.tensor([4, 200, 200, 515], dtype=torch.int64, device=DEV)
    src, dst, rowptr = K.sorted_edges(rng, rows, 3000, hub=True)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    topo = GraphTopology.from_sorted(_dev(rowptr), _dev(src), _dev(dst), rows, status, True)
    base = {"x": rng.standard_normal((rows, C)).astype(np.float32), "e": rng.standard_normal((src.shape[0], De)).astype(np.float32),
            "s1": rng.standard_normal(rows).astype(np.float32), "s2": rng.standard_normal(rows).astype(np.float32)}
    ref1 = P.ref_padded(base["s1"], gp.tolist(), 0.5, src, dst, rowptr)
    n1 = ref1["n_out"]
    results = {}
    for padded in (False, True):
        leaf = {k: _dev(v).requires_grad_(True) for k, v in base.items()}

        def scores2_of(n):  # the sized layer scores its N' rows; the padded one all rows, the slack rows with the best scores of all
            tail = torch.full((n - n1,), 1e9, device=DEV)
            return torch.cat([leaf["s2"][:n1], tail])

        first, second = _pool_twice(padded, leaf["x"], topo, leaf["e"], gp, leaf["s1"], scores2_of)
        n2, e2_count = (second[0].size(0), second[1].size(0)) if not padded else results[False]["sizes"]
        gx = torch.from_numpy(np.random.default_rng(9).standard_normal((n2, C)).astype(np.float32)).to(DEV)
        ge = torch.from_numpy(np.random.default_rng(10).standard_normal((e2_count, De)).astype(np.float32)).to(DEV)
        if padded:  # upstream gradient rows behind N'' / E'': large and finite
            gx = torch.cat([gx, torch.full((rows - n2, C), BIG, device=DEV)])
            ge = torch.cat([ge, torch.full((src.shape[0] - e2_count, De), BIG, device=DEV)])
        ((second[0] * gx).sum() + (second[1] * ge).sum()).backward()
        results[padded] = {"first": first, "second": second, "grads": {k: v.grad for k, v in leaf.items()}, "sizes": (n2, e2_count)}
    (sx1, se1, st1, sgp1, sk1), (sx2, se2, st2, sgp2, sk2) = results[False]["first"], results[False]["second"]
    (px1, pe1, pt1, pgp1, pk1), (px2, pe2, pt2, pgp2, pk2) = results[True]["first"], results[True]["second"]
    n2, e2_count = results[False]["sizes"]
    assert sx1.size(0) == n1 and 0 < n2 < n1 < rows and 0 < e2_count < se1.size(0) < src.shape[0]
    assert pt1.status is topo.status and pt1.deferred and pt2.num_nodes == rows and pt2.num_edges == src.shape[0]
    for sized_t, padded_t, n in ((sx1, px1, n1), (sx2, px2, n2), (se1, pe1, se1.size(0)), (se2, pe2, e2_count)):
        assert padded_t.size(0) in (rows, src.shape[0]) and torch.equal(padded_t[:n], sized_t) and _positive_zero(padded_t[n:].detach())
    assert torch.equal(pgp1, sgp1) and torch.equal(pgp2, sgp2) and int(pgp2[-1]) == n2
    assert torch.equal(pk1[:n1], sk1) and bool((pk1[n1:] == -1).all()) and torch.equal(pk2[:n2], sk2) and bool((pk2[n2:] == -1).all())
    for name in ("src_sorted", "dst_sorted"):
        assert torch.equal(getattr(pt2, name)[:e2_count], getattr(st2, name))
    assert torch.equal(pt2.rowptr[:n2 + 1], st2.rowptr) and int(pt2.rowptr[-1]) == src.shape[0]
    assert bool((pt2.dst_sorted[e2_count:] >= n2).all()) and torch.equal(pt2.dst_sorted[e2_count:], pt2.src_sorted[e2_count:])
    # the composed kept set: -1 must not index
    composed_sized = sk1[sk2.long()]
    composed = torch.where(pk2 >= 0, pk1[pk2.clamp(min=0).long()], pk2)
    assert torch.equal(composed[:n2], composed_sized) and bool((composed[n2:] == -1).all())
    for k, g in results[False]["grads"].items():
        assert torch.equal(results[True]["grads"][k], g), k
    assert all(bool(g.any()) for g in results[False]["grads"].values())
    # nodes only (behind the last block): no topology, the same rows, kept written over its whole length
    from graphnet_classifier_amd import functional as Fn
    x3, e3, topo3, gp3, kept3 = Fn.topk_pool(_dev(base["x"]), _dev(base["s1"]), topo, gp, 0.5, None, need_edges=False, padded=True)
    assert e3 is None and topo3 is None and torch.equal(x3, px1.detach()) and torch.equal(kept3, pk1) and torch.equal(gp3, pgp1)
