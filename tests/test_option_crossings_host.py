"""Host-only: the conditions (a) - (g) of tests/option_crossing_cases.py on every row of ``CROSSINGS``, in the oracle alone, with
one printed line of figures per crossing (quotes them); the composition against what it must reduce to (a
zeroed attention gate: the mean composition; no pooling layer: ``O.graphnet_forward`` under the same ``_scatter``); and the pooled
graph without edges under every aggregation."""
import itertools

import numpy as np
import pytest
import torch

from oracle import graphnet_oracle as O
from tests import option_crossing_cases as X
from tests import segment_reduce_cases as R
from tests import test_gpu_topk_pool_model as M
from tests._util import max_abs


def test_the_table_covers_every_crossing():
    product = set(itertools.product(X.AGGREGATIONS, X.READOUTS))
    assert {(c.aggregation, c.readout) for c in X.FORWARD_ROWS} == product and len(X.FORWARD_ROWS) == len(product)
    assert {(c.aggregation, c.readout) for c in X.GRADIENT_ROWS} == product and len(X.GRADIENT_ROWS) == len(product)
    assert all(set(c.inputs) == set(X.FORWARD_INPUTS) for c in X.FORWARD_ROWS)
    assert all(X.SMALLEST in c.inputs for c in X.GRADIENT_ROWS)
    assert len({c.id for c in X.CROSSINGS}) == len(X.CROSSINGS)


@pytest.mark.parametrize("crossing", X.CROSSINGS, ids=lambda c: c.id)
def test_the_seed_meets_the_conditions(crossing):
    c = crossing
    f = X.crossing_figures(c)
    s = X.summary(c, f)
    print(f"{c.id}: gap ratio (a) {s['gap_ratio']:.0f}, first k (b) {s['first_k']}, apart (c) {s['apart']:.2e}, fp32 vs float64 (d) "
          f"{s['fp32_vs_f64']:.1e}, winner gap (e) {s['winner_gap']}, isolated (f) {f['isolated']}, vs mean (g) {s['vs_mean']}")
    for g in f["layers"]:
        assert np.isfinite(g["score_err"]) and g["min_gap"] >= 100.0 * g["score_err"], g  # (a)
        assert not g["first_k"], g                                                        # (b)
        assert g["apart"] >= 10 * X.BAR, g                                                # (c)
    assert all(v <= 0.5 * X.BAR for v in f["fp32_vs_f64"].values()), f["fp32_vs_f64"]    # (d)
    if c.aggregation == "max" and c.gradients:                                            # (e)
        assert f["winner_gap"][X.SMALLEST] >= X.MIN_GAP, f["winner_gap"]
    # (f) an empty destination on a pooled rowptr - in the forward somewhere, and in the graph whose gradients are compared
    assert s["isolated"] >= 1 and (not c.gradients or s["isolated_smallest"] >= 1), f["isolated"]
    if c.aggregation != "mean":                                                           # (g)
        assert s["vs_mean"] > 200 * X.BAR, f["vs_mean"]


def _small(aggregation, readout="mean", dtype=torch.float64):
    x, pos, ei = M._graph(20)
    m = M._model(readout, seed=0, aggregation=aggregation)
    return m, x.to(dtype), pos.to(dtype), ei


def test_a_zeroed_attention_gate_is_the_mean_composition():
    """Equal scores: every weight is 1 / deg, and the crossed attention oracle is the crossed mean oracle - the same kept nodes and
    the same logits, exactly."""
    m, x, pos, ei = _small("attention")
    with torch.no_grad():
        for block in m.graph_net.graph_processor.blocks:
            block.node_model.gate.model[2].weight.zero_()
            block.node_model.gate.model[2].bias.zero_()
    sd = X.state(m, torch.float64)
    alphas = []
    att, kept_att = X.crossed_logits("attention", sd, x, pos, ei, X.RATIO, X.POOL_AFTER, "mean", alphas=alphas)
    mean, kept_mean = X.crossed_logits("mean", sd, x, pos, ei, X.RATIO, X.POOL_AFTER, "mean")
    print(f"zeroed gate: |attention - mean composition| = {max_abs(att, mean):.1e}")
    assert np.array_equal(kept_att, kept_mean) and torch.equal(att, mean)
    assert len(alphas) == X.N_BLOCKS and alphas[0].numel() == ei.size(1) and 0 < alphas[1].numel() < ei.size(1)
    deg = torch.bincount(ei[1], minlength=x.size(0)).double()
    assert max_abs(alphas[0], 1.0 / deg[ei[1]]) <= 1e-15


@pytest.mark.parametrize("aggregation", ("sum",) + X.AGGREGATIONS)
def test_without_a_pooling_layer_it_is_the_plain_oracle(aggregation):
    m, x, pos, ei = _small(aggregation, dtype=torch.float32)
    sd = X.state(m)
    got, kept = X.crossed_logits(aggregation, sd, x, pos, ei, X.RATIO, (), "mean")
    with X.oracle_scatter(aggregation, sd):
        want = O.classifier_forward(sd, O.graphnet_forward(sd, x, pos, ei, prefix="graph_net.").mean(0))
    assert O._scatter is O.scatter_sum_fast  # and the oracle is itself again
    assert torch.equal(got[0], want) and kept.tolist() == list(range(x.size(0)))
    pooled, _ = X.crossed_logits(aggregation, sd, x, pos, ei, X.RATIO, X.POOL_AFTER, "mean")
    assert max_abs(pooled[0], want) >= 10 * X.BAR


@pytest.mark.parametrize("aggregation", ("sum",) + X.AGGREGATIONS)
def test_the_pooled_graph_without_edges(aggregation):
    """Rows 0 .. 19 and then 0 .. 9 survive, no edge does, every block calls ``_scatter`` once (block b scores with gate b: the
    second call sees no rows), and fp32 stays within half a bar of float64."""
    m, x, pos, ei = X.edgeless_case(aggregation)
    sd, sd64 = X.state(m), X.state(m, torch.float64)
    rec, alphas = [], []
    R.MAX_GAPS.clear()
    R.RECORD_GAPS = aggregation == "max"
    try:
        l64, kept = X.crossed_logits(aggregation, sd64, x.double(), pos.double(), ei, X.RATIO, X.POOL_AFTER, "mean", record=rec, alphas=alphas)
    finally:
        R.RECORD_GAPS = False
    l32, kept32 = X.crossed_logits(aggregation, sd, x, pos, ei, X.RATIO, X.POOL_AFTER, "mean")
    assert kept.tolist() == kept32.tolist() == list(range(10))
    first = rec[0][2]
    assert first.tolist() == [True] * 20 + [False] * 20 and not bool((first[ei[0].numpy()] & first[ei[1].numpy()]).any())  # E' = 0
    assert X.isolated_after_first_pool(ei, first) == 20
    assert rec[1][0].numel() == 20 and float(rec[1][0].min()) == float(rec[1][0].max())
    print(f"edge-less, {aggregation}: |fp32 - float64 oracle| = {max_abs(l32, l64):.1e}, winner gaps {R.MAX_GAPS}")
    assert max_abs(l32, l64) <= 0.5 * X.BAR
    if aggregation == "attention":
        assert [a.numel() for a in alphas] == [90, 0]
    if aggregation == "max":  # one call with candidates (block 1 of 2); the block without edges has none to tell apart
        assert len(R.MAX_GAPS) == 1
        assert X.EDGELESS_MAX_GRADIENTS_COMPARED == (R.MAX_GAPS[0] >= X.MIN_GAP)
    ref = X.reference_gradients(m, aggregation, "mean", x, pos, ei)
    assert set(ref) == set(sd) and all(bool(torch.isfinite(g).all()) for g in ref.values())
    dead = [k for k, g in ref.items() if not bool(g.any())]
    # the survivors (rows 0 .. 19) never had an incoming edge, so nothing on the edge path is reached - the second block's edge model
    # is not even run - while both node processors see their all-zero aggregates
    assert all(k in dead for k in ref if ".edge_model." in k or ".edge_encoder." in k or ".node_model.gate." in k), dead
    assert not any(".node_model.node_processor." in k or ".node_encoder." in k or ".pools.1.gate.model.2." in k for k in dead), dead
