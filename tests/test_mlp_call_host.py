"""CPU: the flat argument layout of a fused-MLP call, through the public entry ``functional.fused_mlp``: what reaches
``_FusedMLP.apply`` is tables, weights, biases, gamma, beta, residual in that order, and ``rows`` defaults to the first segment's
row count.  Every combination of 1..4 segments, 1..3 Linear layers, LayerNorm or none, residual or none."""
import itertools
import types

import pytest
import torch

from graphnet_classifier_amd import functional as Fn

CASES = list(itertools.product((1, 2, 3, 4), (1, 2, 3), (False, True), (False, True)))
IDS = [f"s{s}_l{l}{'_ln' if ln else ''}{'_res' if res else ''}" for s, l, ln, res in CASES]
ROWS, TABLE_ROWS, HIDDEN, OUT = 5, 7, 6, 4
G = object()  # stands for a gradient


def _call(s, l, has_ln, has_res, gathered_first):
    """CPU operands of one call: segment k is [TABLE_ROWS, k + 2] wide; odd segments (and the first, when asked) are gathered."""
    tables = [torch.zeros(TABLE_ROWS, k + 2) for k in range(s)]
    indices = [torch.zeros(ROWS, dtype=torch.int32) if (k % 2 == 1 or (k == 0 and gathered_first)) else None for k in range(s)]
    widths = [sum(t.size(1) for t in tables)] + [HIDDEN] * (l - 1) + [OUT]
    weights = [torch.zeros(widths[k + 1], widths[k]) for k in range(l)]
    biases = [torch.zeros(widths[k + 1]) for k in range(l)]
    ln = (torch.ones(OUT), torch.zeros(OUT), 1e-5) if has_ln else None
    residual = torch.zeros(ROWS, OUT) if has_res else None
    return list(zip(tables, indices)), weights, biases, ln, residual


def _expected_flat(segments, weights, biases, ln, residual):
    return [t for t, _ in segments] + weights + biases + (list(ln[:2]) if ln is not None else []) + ([residual] if residual is not None else [])


def _same(got, want):
    return len(got) == len(want) and all(a is b for a, b in zip(got, want))


@pytest.mark.parametrize("s,l,has_ln,has_res", CASES, ids=IDS)
def test_flat_order_and_default_rows_at_the_public_entry(monkeypatch, s, l, has_ln, has_res):
    seen = []
    monkeypatch.setattr(Fn._FusedMLP, "apply", staticmethod(lambda meta, *args: seen.append((meta, args))))
    for gathered_first in (False, True):
        segments, weights, biases, ln, residual = _call(s, l, has_ln, has_res, gathered_first)
        Fn.fused_mlp(segments, weights, biases, ln=ln, activation="Tanh", act_param=0.25, residual=residual)
        meta, args = seen.pop()
        assert _same(args, _expected_flat(segments, weights, biases, ln, residual))
        # rows: the first segment's index length when it is gathered, its table's rows otherwise
        assert meta.rows == (ROWS if gathered_first else TABLE_ROWS)
        assert _same(meta.indices, [i for _, i in segments])
        assert (meta.activation, meta.act_param, meta.num_linear) == ("Tanh", 0.25, l)
        assert meta.ln_eps == (1e-5 if has_ln else 0.0)
        Fn.fused_mlp(segments, weights, biases, ln=ln, residual=residual, rows=3)
        meta, args = seen.pop()
        assert meta.rows == 3 and _same(args, _expected_flat(segments, weights, biases, ln, residual))


def _named_slots(call):
    """(keyword arguments of ``call.grads`` that place ONE gradient, the group and position it belongs to) for every slot."""
    s, l = call.num_tables, call.num_linear
    for group, n in (("tables", s), ("weights", l), ("biases", l)):
        for k in range(n):
            yield {group: [G if j == k else None for j in range(n)]}, (group, k)
    for name in (("gamma", "beta") if call.has_ln else ()) + (("residual",) if call.has_residual else ()):
        yield {name: G}, (name, None)


def _check_record(call, flat, tables, weights, biases, ln, residual):
    """pack / unpack are inverse to each other on ``flat``, and a gradient placed by name lands where its argument is in ``flat``
    (autograd pairs the returned tuple with the arguments by position)."""
    assert _same(call.pack(tables, weights, biases, ln, residual), flat)
    a = call.unpack(flat)
    assert _same(a.tables, tables) and _same(a.weights, weights) and _same(a.biases, biases) and a.residual is residual
    assert (a.ln is None) == (ln is None) and (ln is None or (a.ln[0] is ln[0] and a.ln[1] is ln[1] and a.ln[2] == ln[2]))
    assert _same(call.pack(*a), flat)
    args, rest = call.split_saved(tuple(flat) + ("p", "q"))
    assert _same(args, flat) and rest == ["p", "q"]
    every = [True] * len(flat)
    assert call.grads(every) == (None,) * len(flat)
    named = {"tables": tables, "weights": weights, "biases": biases, "gamma": ln and ln[0], "beta": ln and ln[1], "residual": residual}
    slots = list(_named_slots(call))
    assert len(slots) == len(flat)
    for kwargs, (group, k) in slots:
        argument = named[group] if k is None else named[group][k]
        where = [i for i, f in enumerate(flat) if f is argument]
        assert len(where) == 1
        got = call.grads(every, **kwargs)
        assert len(got) == len(flat) and [i for i, g in enumerate(got) if g is G] == where and got.count(None) == len(flat) - 1
        assert call.grads([i not in where for i in range(len(flat))], **kwargs) == (None,) * len(flat)  # not needed: None


@pytest.mark.parametrize("s,l,has_ln,has_res", CASES, ids=IDS)
def test_record_round_trip_and_gradients_by_name(monkeypatch, s, l, has_ln, has_res):
    seen = []
    monkeypatch.setattr(Fn._FusedMLP, "apply", staticmethod(lambda call, *flat: seen.append((call, flat))))
    segments, weights, biases, ln, residual = _call(s, l, has_ln, has_res, False)
    Fn.fused_mlp(segments, weights, biases, ln=ln, residual=residual)
    call, flat = seen.pop()
    _check_record(call, flat, [t for t, _ in segments], weights, biases, ln, residual)


@pytest.mark.parametrize("with_agg", [False, True])
@pytest.mark.parametrize("l,has_ln", [(l, ln) for l in (1, 2, 3) for ln in (False, True)])
def test_wsplit_record_has_the_layout_x_e_params(monkeypatch, l, has_ln, with_agg):
    seen = []
    monkeypatch.setattr(Fn._EdgeProcessorWSplit, "apply", staticmethod(lambda call, topo, *flat: seen.append((call, topo, flat))))
    (_, weights, biases, ln, _), x, e = _call(1, l, has_ln, False, False), torch.zeros(TABLE_ROWS, 8), torch.zeros(ROWS, OUT)
    topo = types.SimpleNamespace(src_sorted=torch.zeros(ROWS, dtype=torch.int32), dst_sorted=torch.ones(ROWS, dtype=torch.int32))
    Fn.edge_processor_wsplit(x, e, topo, weights, biases, ln, "ReLU", 0.0, with_agg=with_agg)
    call, got_topo, flat = seen.pop()
    assert got_topo is topo and _same(flat, [x, e] + weights + biases + (list(ln[:2]) if has_ln else []))
    assert call.with_agg is with_agg and call.rows == ROWS and not call.has_residual
    assert call.indices[0] is topo.src_sorted and call.indices[1] is topo.dst_sorted
    _check_record(call, flat, [x, e], weights, biases, ln, None)
