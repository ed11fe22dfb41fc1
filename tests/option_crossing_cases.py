"""Top-K node pooling (K20) crossed with every neighbourhood aggregation (K18 mean / max, K21 attention) and read-out (K17 mean, K19
attention): the composed reference, the table of crossings and the conditions on their seeds.  No GPU here; shared by
tests/test_option_crossings_host.py and tests/test_gpu_option_crossings_model.py.

Nothing is restated: the reference is ``topk_pool_cases.pooled_logits`` with ``oracle.graphnet_oracle._scatter`` replaced for the
duration of one call by ``segment_reduce_cases.ORACLE_SCATTER["mean" | "max"]`` or a fresh
``segment_softmax_cases.OracleAttentionScatter`` (``crossed_logits``); the model is ``test_gpu_topk_pool_model._model``; the
per-layer figures are ``test_gpu_topk_pool_model._figures_of`` over that reference.

The conditions a crossing's seed has to meet (``crossing_figures`` computes the quantities from the oracle alone and
tests/test_option_crossings_host.py asserts them):
 (a) at every pooling layer and graph the float64 gap between the k-th and the (k + 1)-th score is at least 100 x the measured
     |fp32 oracle - float64 oracle| of that layer's scores, and fp32 and float64 keep the same nodes;
 (b) the kept set is not the first k rows;
 (c) the pooled float64 logits differ from the un-pooled ones of the same weights by at least ten bars (1e-4) on every graph;
 (d) the fp32 oracle's logits are within half the 1e-5 bar of the float64 oracle's;
 (e) ``"max"``, where gradients are compared: the smallest winner gap is at least ``MIN_GAP``;
 (f) behind the first pooling layer - the topology the second block runs on; nothing reads the one behind the last block - at
     least one kept node has no incoming kept edge, on some input and, where gradients are compared, on the 69-node graph;
 (g) ``"max"`` and ``"attention"``: the pooled float64 logits differ from those of the mean model on the same weights by more than
     200 bars on some input (the rule of K21: with either model within a bar of its oracle, no mean passes for the other).
"""
import contextlib
from dataclasses import dataclass

import numpy as np
import torch

from oracle import graphnet_oracle as O
from tests import segment_reduce_cases as R
from tests import segment_softmax_cases as S
from tests import test_gpu_topk_pool_model as M
from tests import topk_pool_cases as K
from tests._util import max_abs

BAR = 1e-5
MIN_GAP = 1e-4
RATIO, POOL_AFTER, N_BLOCKS = M.RATIO, (0, 1), 2
AGGREGATIONS = ("mean", "max", "attention")
READOUTS = M.READOUTS
SMALLEST = "69 nodes"  # the graph of the gradient comparisons
FORWARD_INPUTS = ("69 nodes", "119 nodes", "100 nodes", "batch of six")  # the names of ``M._inputs()``


@dataclass(frozen=True)
class Crossing:
    aggregation: str
    readout: str
    seed: int
    inputs: tuple      # names of ``M._inputs()`` the forward is compared on
    gradients: bool    # the gradients are compared too, on the 69-node graph (which is then among ``inputs``)

    @property
    def id(self) -> str:
        return f"{self.aggregation}-{self.readout}-seed{self.seed}-{'forward+gradients' if self.gradients else 'forward'}"


# The float64 gradient reference of a max needs a winner gap (e), which no seed offers on the batch of six; its forward, continuous
# in the candidates, does not.  So the max crossings have two rows each: forward on every input, gradients on the 69-node graph.
CROSSINGS = (
    Crossing("mean", "mean", 0, FORWARD_INPUTS, True),
    Crossing("mean", "attention", 0, FORWARD_INPUTS, True),
    Crossing("attention", "mean", 463, FORWARD_INPUTS, True),
    Crossing("attention", "attention", 463, FORWARD_INPUTS, True),
    Crossing("max", "mean", 42, FORWARD_INPUTS, False),
    Crossing("max", "attention", 42, FORWARD_INPUTS, False),
    Crossing("max", "mean", 25, (SMALLEST,), True),
    Crossing("max", "attention", 25, (SMALLEST,), True),
)
FORWARD_ROWS = tuple(c for c in CROSSINGS if len(c.inputs) > 1)
GRADIENT_ROWS = tuple(c for c in CROSSINGS if c.gradients)

# The pooled graph without edges (``edgeless_case``): are the max model's gradients compared with float64 autograd?  Only if the
# smallest winner gap of its blocks is at least MIN_GAP; tests/test_option_crossings_host.py asserts that this constant says so.
EDGELESS_SEED = M.SEED
EDGELESS_MAX_GRADIENTS_COMPARED = False


# ---------------------------------------------------------------------------------------------------------------- reference
def _max_or_zeros(src, index, dim_size):
    """``ORACLE_SCATTER["max"]``; a block without edges (no candidates at all) aggregates to zeros."""
    if src.size(0) == 0:
        return src.new_zeros((dim_size, src.size(1)))
    return R.ORACLE_SCATTER["max"](src, index, dim_size)


class _AttentionOrZeros(S.OracleAttentionScatter):
    """A block without edges has no row to score (``O.mlp_forward`` cannot take an empty table): the call is still counted, so that
    block b keeps gate b, its weights are an empty vector and the aggregate is zeros."""

    def __call__(self, src, index, dim_size):
        if src.size(0):
            return super().__call__(src, index, dim_size)
        self.calls += 1
        self.alphas.append(src.new_zeros(0))
        return src.new_zeros((dim_size, src.size(1)))


@contextlib.contextmanager
def oracle_scatter(aggregation: str, sd: dict):
    """``O._scatter`` replaced for one forward in the dtype of ``sd``; yields the fresh ``OracleAttentionScatter`` (else None)."""
    before = O._scatter
    scatter = None
    if aggregation == "sum":  # the ATen form is the differentiable one
        O.set_scatter_impl("index_add" if any(v.requires_grad for v in sd.values()) else "sorted_loop")
    elif aggregation == "attention":
        scatter = O._scatter = _AttentionOrZeros(sd)
    else:
        O._scatter = _max_or_zeros if aggregation == "max" else R.ORACLE_SCATTER[aggregation]
    try:
        yield scatter
    finally:
        O._scatter = before


def crossed_logits(aggregation, sd, x, pos, ei, ratio, pool_after, readout, graph_ptr=None, record=None, alphas=None):
    """``K.pooled_logits`` under ``aggregation``: ``(logits [G, classes], kept)``.  The attention stand-in picks block b's gate by
    counting calls, and every block - with edges (``O.gn_block``) or without (``O.node_processor`` alone) - calls it once: asserted
    after the forward.  ``alphas``: a list that receives the per-block weights."""
    with oracle_scatter(aggregation, sd) as scatter:
        out = K.pooled_logits(sd, x, pos, ei, ratio, pool_after, readout, graph_ptr, record=record)
    if scatter is not None:
        assert scatter.calls == len(scatter.alphas) == O.n_blocks_of(sd, "graph_net.") == N_BLOCKS
        if alphas is not None:
            alphas.extend(scatter.alphas)
    return out


def state(m, dtype=torch.float32, grad=False):
    sd = M._sd(m, dtype)
    return {k: v.requires_grad_(True) for k, v in sd.items()} if grad else sd


def reference_gradients(m, aggregation, readout, x, pos, ei, label=None):
    """float64 autograd of the composition: {name: gradient}, zeros for a parameter the forward never reaches (the edge model of
    a block without edges).  ``label`` None: the loss is the sum of the logits."""
    sd = state(m, torch.float64, grad=True)
    logits, _ = crossed_logits(aggregation, sd, x.double(), pos.double(), ei, RATIO, POOL_AFTER, readout)
    loss = logits.sum() if label is None else torch.nn.functional.cross_entropy(logits, label[None])
    loss.backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------------------ figures
def isolated_after_first_pool(ei, keep) -> int:
    """Kept nodes without an incoming kept edge behind the first pooling layer (``keep``: bool [N] numpy)."""
    src, dst = ei[0].numpy(), ei[1].numpy()
    alive = keep[src] & keep[dst]
    return int((keep & (np.bincount(dst[alive], minlength=keep.size) == 0)).sum())


def crossing_figures(c: Crossing) -> dict:
    """From the oracle alone: ``layers`` - the dicts of ``M._figures_of`` per (input, pooling layer, graph): ``min_gap``,
    ``score_err`` (inf when fp32 and float64 keep different nodes), ``first_k``, ``apart``; per input name ``fp32_vs_f64`` (d),
    ``isolated`` (f), ``vs_mean`` (g; None for the mean aggregation) and ``winner_gap`` (e; None unless ``"max"``)."""
    inputs = [i for i in M._inputs() if i[0] in c.inputs]
    assert len(inputs) == len(c.inputs)
    m = M._model(c.readout, seed=c.seed, aggregation=c.aggregation)
    sd, sd64 = state(m), state(m, torch.float64)

    def logits_of(sd_, *args, **kw):
        return crossed_logits(c.aggregation, sd_, *args, **kw)

    out = {"layers": M._figures_of(sd, sd64, c.readout, c.aggregation, inputs, logits=logits_of),
           "fp32_vs_f64": {}, "isolated": {}, "vs_mean": {}, "winner_gap": {}}
    for name, x, pos, ei, gp in inputs:
        rec = []
        R.MAX_GAPS.clear()
        R.RECORD_GAPS = c.aggregation == "max"
        try:
            l64, _ = logits_of(sd64, x.double(), pos.double(), ei, RATIO, POOL_AFTER, c.readout, gp, record=rec)
        finally:
            R.RECORD_GAPS = False
        out["winner_gap"][name] = min(R.MAX_GAPS) if c.aggregation == "max" else None
        l32, _ = logits_of(sd, x, pos, ei, RATIO, POOL_AFTER, c.readout, gp)
        out["fp32_vs_f64"][name] = max_abs(l32, l64)
        out["isolated"][name] = isolated_after_first_pool(ei, rec[0][2])
        out["vs_mean"][name] = None
        if c.aggregation != "mean":
            mean, _ = crossed_logits("mean", sd64, x.double(), pos.double(), ei, RATIO, POOL_AFTER, c.readout, gp)
            out["vs_mean"][name] = max_abs(l64, mean)
    return out


def summary(c: Crossing, f: dict) -> dict:
    """The worst of every figure of a crossing: what the conditions are asserted on and DESIGN.md quotes."""
    ratios = [(g["min_gap"] / g["score_err"] if g["score_err"] > 0 else float("inf")) for g in f["layers"] if np.isfinite(g["min_gap"])]
    return {"gap_ratio": min(ratios), "same_nodes": all(np.isfinite(g["score_err"]) for g in f["layers"]),
            "first_k": any(g["first_k"] for g in f["layers"]), "apart": min(g["apart"] for g in f["layers"]),
            "fp32_vs_f64": max(f["fp32_vs_f64"].values()), "isolated": sum(f["isolated"].values()),
            "isolated_smallest": f["isolated"].get(SMALLEST, 0),
            "vs_mean": max(f["vs_mean"].values()) if c.aggregation != "mean" else None,
            "winner_gap": min(f["winner_gap"].values()) if c.aggregation == "max" else None}


# -------------------------------------------------------------------------------------------------- the graph that loses its edges
def edgeless_case(aggregation: str, readout: str = "mean"):
    """``(model, x, pos, ei)`` of test_a_pooled_graph_without_edges_runs_the_remaining_blocks under ``aggregation``: 40 nodes whose
    90 edges lie among the ids 20 .. 39, every scorer's last weight zeroed and its bias 0.7 - all scores are equal, the tie rule
    keeps rows 0 .. 19 and then 0 .. 9 on both sides, and the second block runs on E' = 0."""
    rng = np.random.default_rng(2)
    n = 40
    x = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    pos = torch.from_numpy(rng.standard_normal((n, 2)).astype(np.float32))
    ei = torch.from_numpy(rng.integers(20, 40, size=(2, 90)))
    m = M._model(readout, seed=EDGELESS_SEED, **({} if aggregation == "sum" else {"aggregation": aggregation}))
    with torch.no_grad():
        for pool in m.graph_net.graph_processor.pools.values():
            pool.gate.model[2].weight.zero_()
            pool.gate.model[2].bias.fill_(0.7)
    return m, x, pos, ei
