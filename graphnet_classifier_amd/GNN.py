"""Drop-in for the reference's ``models/GNN.py``: same public names, constructors, kwargs
defaults and ``state_dict`` layout; the forward path runs in hand-written HIP kernels
(CSR scatter-sum K1, fused gather+concat+MLP+LayerNorm+residual K4, edge features K6).

Reference: models/GNN.py:3-341.  Differences that are deliberate and documented in
DESIGN.md: inside ``GraphNet``/``GraphProcessor`` the edge latents are kept in
destination-sorted order (a stable sort, so every per-destination sum adds in the
reference's edge order), and inputs given on the CPU are moved to the module's GPU and the
result moved back, because the reference's callers (utils/train_model.py:37,
utils/inference.py:59) never place tensors themselves.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
from torch import Tensor

from . import functional as Fn
from . import native
from .MLP import MLP, default_device, require_gpu_param
from .topology import GraphTopology, get_destination_csr, get_topology


# Algebraic split of the edge processor's first Linear (DESIGN.md, K4 "W-split"); GNC_NO_WSPLIT=1
# keeps the reference-form concat for A/B measurements.
WSPLIT = os.environ.get("GNC_NO_WSPLIT") is None
# A/B switch: GNC_NO_READOUT_KERNEL=1 leaves the read-out classifier (one graph, or the G graphs of forward_batched) to PyTorch-ROCm
# (3 GEMM + 2 clamp + copies; batched with graph_ptr also an index gather and a product that store a [G, F] feature matrix)
READOUT_HIP = os.environ.get("GNC_NO_READOUT_KERNEL") is None
# Inference: the edge processor's launch also forms the node model's per-destination sums (fused aggregation
# epilogue); GNC_NO_FUSED_AGG=1 keeps K1 as a separate launch for A/B measurements.
FUSED_AGG = os.environ.get("GNC_NO_FUSED_AGG") is None
# Inference: GraphNet.forward_device drops the last GN block's edge output, so that block's edge launch forms only the
# aggregate and stores no e' rows (gnc_mlp_forward_agg_only_f32); GNC_NO_DEAD_EDGE_STORE=1 keeps the storing launch for A/B.
DROP_DEAD_EDGE_STORE = os.environ.get("GNC_NO_DEAD_EDGE_STORE") is None


# --------------------------------------------------------------------------- a1 scatter_sum
def scatter_sum(src: Tensor, index: Tensor, dim: int = 0, dim_size: int | None = None) -> Tensor:
    """Operator-level seam of the reference (models/GNN.py:4-21), same signature and errors.

    ``src`` rows may be in any order; the destination CSR for ``index`` is built (or taken from
    the topology cache) and the sum runs in the atomics-free HIP kernel.  ``dim_size=None``
    costs a host sync exactly like the reference's ``index.max().item()``."""
    if dim != 0:
        raise NotImplementedError("fallback scatter_sum currently supports dim=0 only")
    if src.ndim == 1:
        src = src.unsqueeze(-1)
    if dim_size is None:
        dim_size = int(index.max().item()) + 1 if index.numel() > 0 else 0
    dev = src.device if src.is_cuda else default_device()
    if dev.type != "cuda":
        raise RuntimeError("scatter_sum: no GPU visible and no CPU fallback exists")
    out_device = src.device
    csr = get_destination_csr(index, dim_size, dev)  # destination sort of `index` only; cached on the tensor itself
    src = src.to(device=dev, dtype=torch.float32)
    out = Fn.scatter_sum_csr(src, csr.rowptr, csr.perm, csr.col32 if src.requires_grad else None, dim_size)
    return out if out_device == dev else out.to(out_device)


def _scatter_args(who: str, src: Tensor, index: Tensor, dim: int, dim_size: int | None):
    """The argument handling ``scatter_sum`` has, for its mean / max siblings: (src [E, D] on the GPU, csr, dim_size, the device
    the result goes back to, the device it is computed on)."""
    if dim != 0:
        raise NotImplementedError(f"fallback {who} currently supports dim=0 only")
    if src.ndim == 1:
        src = src.unsqueeze(-1)
    if dim_size is None:
        dim_size = int(index.max().item()) + 1 if index.numel() > 0 else 0
    dev = src.device if src.is_cuda else default_device()
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: no GPU visible and no CPU fallback exists")
    out_device = src.device
    csr = get_destination_csr(index, dim_size, dev)
    return src.to(device=dev, dtype=torch.float32), csr, dim_size, out_device, dev


def scatter_mean(src: Tensor, index: Tensor, dim: int = 0, dim_size: int | None = None) -> Tensor:
    """``scatter_sum``'s sibling (same signature, argument handling and errors): out[v] = mean of the ``src`` rows with
    ``index == v`` - their sum in row order divided by their count - and +0.0 for a ``v`` without rows (K18)."""
    src, csr, dim_size, out_device, dev = _scatter_args("scatter_mean", src, index, dim, dim_size)
    out = Fn.segment_mean_csr(src, csr.rowptr, csr.perm, csr.col32 if src.requires_grad else None, dim_size)
    return out if out_device == dev else out.to(out_device)


def scatter_max(src: Tensor, index: Tensor, dim: int = 0, dim_size: int | None = None) -> tuple[Tensor, Tensor]:
    """``(out, argmax)``: out[v] = column-wise maximum of the ``src`` rows with ``index == v``, +0.0 for a ``v`` without rows; a
    NaN wins its column; ``-0.0 == +0.0``.  ``argmax`` [dim_size, D] int64 is the row of ``src`` that holds each maximum - the
    LOWEST such row on a tie - and -1 for a ``v`` without rows (torch_scatter's ``scatter_max`` puts ``src.size(0)`` there
    instead).  The gradient of a column goes to that row alone (K18)."""
    src, csr, dim_size, out_device, dev = _scatter_args("scatter_max", src, index, dim, dim_size)
    out, argmax = Fn.segment_max_csr(src, csr.rowptr, csr.perm, csr.col32 if src.requires_grad else None, dim_size,
                                     return_argmax=True)
    argmax = argmax.long()
    return (out, argmax) if out_device == dev else (out.to(out_device), argmax.to(out_device))


def scatter_attention(src: Tensor, scores: Tensor, index: Tensor, dim: int = 0, dim_size: int | None = None) -> Tensor:
    """``scatter_mean``'s learned sibling (same argument handling and errors): out[v] = sum of alpha_r src[r] over the rows with
    ``index == v``, ``alpha`` the softmax of their ``scores`` (one float per row of ``src``) - in row order, +0.0 for a ``v`` without
    rows; equal scores give ``scatter_mean``'s bits (K21)."""
    src, csr, dim_size, out_device, dev = _scatter_args("scatter_attention", src, index, dim, dim_size)
    if scores.numel() != src.size(0):
        raise ValueError(f"scatter_attention: {scores.numel()} scores for {src.size(0)} rows of src")
    scores = scores.reshape(-1).to(device=dev, dtype=torch.float32)
    need = src.requires_grad or scores.requires_grad
    out = Fn.segment_softmax_csr(src, scores, csr.rowptr, csr.perm, csr.col32 if need else None, dim_size)
    return out if out_device == dev else out.to(out_device)


AGGREGATIONS = ("sum", "mean", "max", "attention")


def _check_aggregation(aggregation, who: str) -> str:
    if aggregation not in AGGREGATIONS:
        raise ValueError(f"{who}: aggregation {aggregation!r} is not one of {AGGREGATIONS}")
    return aggregation


# --------------------------------------------------------------------------- a3 EdgeProcessor
def _poison_if_deferred(topo: GraphTopology, out: Tensor) -> Tensor:
    """Deferred validation (topology.set_validation): the topology's out-of-range flags have not been read back, and the
    kernels ran on sanitised ids - a result computed from a bad ``edge_index`` must not look plausible (the reference raises
    IndexError, models/GNN.py:18-20; ``check_deferred()`` raises it later).  NaN on the device when a flag is set."""
    if not topo.deferred:
        return out
    if out.requires_grad or not out.is_contiguous():
        return torch.where(topo.status.any(), torch.full_like(out, float("nan")), out)
    return native.poison_if_flagged_(out, topo.status)  # inference: one launch that returns at once unless a flag is set


class EdgeProcessor(nn.Module):
    def __init__(self, in_dim_node: int, in_dim_edge: int, hidden_dim: int = 128, hidden_layers: int = 2,
                 activation: str = "ReLU", initializer: None | str = None, norm_type: None | str = "LayerNorm"):
        """models/GNN.py:31-55."""
        super().__init__()
        self.edge_processor = MLP(2 * in_dim_node + in_dim_edge, in_dim_edge, hidden_dim, hidden_layers, activation,
                                  initializer, norm_type)

    def forward(self, src, dest, edge_attr, u=None, batch=None):
        """MetaLayer edge-model contract (models/GNN.py:57-64): MLP(cat[src, dest, e]) + e."""
        dev = require_gpu_param(self.edge_processor.model[0].weight, "EdgeProcessor")
        back = edge_attr.device
        src, dest, edge_attr = (t.to(device=dev, dtype=torch.float32) for t in (src, dest, edge_attr))
        out = self.edge_processor.forward_segments([(src, None), (dest, None), (edge_attr, None)], residual=edge_attr)
        return out if back == dev else out.to(back)

    def forward_sorted(self, x: Tensor, topo: GraphTopology, edge_attr: Tensor, aggregate: bool = False,
                       need_edges: bool = True):
        """Same math with the two row gathers fused into the kernel; ``edge_attr`` and the
        result are in destination-sorted edge order.  ``aggregate=True`` returns ``(e', agg)`` where ``agg`` is the
        per-destination sum of ``e'`` formed in the same launch, or None when this path cannot provide it (the
        caller then runs K1).  ``need_edges=False`` (with ``aggregate``, autograd off): ``e'`` may come back as None
        when the launch can form ``agg`` without storing it."""
        mlp = self.edge_processor
        weights, biases, ln = mlp._kernel_params()
        # (with autograd on, only for ReLU: its backward is the fused K8 launch over the split form; another activation
        # trains through the concat form, whose backward runs layer by layer - functional._layerwise_mlp_backward_hip)
        trainable_split = mlp.activation_name == "ReLU" or not torch.is_grad_enabled()
        if (WSPLIT and trainable_split and mlp.norm_type != "BatchNorm1d" and mlp.activation_name in native.ACTIVATIONS
                and weights[0].size(1) == 2 * x.size(1) + edge_attr.size(1) and x.size(1) % 4 == 0):
            # W-split of the first Linear: node-side products once per node, gathered and added per edge
            if aggregate and not torch.is_grad_enabled():
                return Fn.edge_processor_wsplit_aggregated(x, edge_attr, topo, weights, biases, ln, mlp.activation_name,
                                                           mlp._act_param(), store_edges=need_edges)
            # (with aggregate, training: the same launch, both outputs differentiable)
            return Fn.edge_processor_wsplit(x, edge_attr, topo, weights, biases, ln, mlp.activation_name, mlp._act_param(),
                                            with_agg=aggregate)
        out = mlp.forward_segments(
            [(x, topo.src_sorted), (x, topo.dst_sorted), (edge_attr, None)], residual=edge_attr, rows=topo.num_edges)
        return (out, None) if aggregate else out


# --------------------------------------------------------------------------- a2 NodeProcessor
class NodeProcessor(nn.Module):
    def __init__(self, in_dim_node: int, in_dim_edge: int, hidden_dim: int = 128, hidden_layers: int = 2,
                 activation: str = "ReLU", initializer: None | str = None, norm_type: None | str = "LayerNorm",
                 aggregation: str = "sum", attention_hidden: int | None = None):
        """models/GNN.py:69-93.  ``aggregation``: how the incoming edge latents of a node are reduced - ``"sum"`` (the reference's
        code), ``"mean"`` (the reference's write-up), ``"max"`` (K18) or ``"attention"`` (K21).  For the first three a plain
        attribute: no parameter, no buffer, not in the ``state_dict``.  ``"attention"`` adds ``self.gate``, the score of an edge
        latent: ``W2 relu(W1 e' + b1) + b2`` with ``attention_hidden`` (32) hidden units - ``TopKPool.gate``'s shape, on the
        fused-MLP kernels over the E rows; a node's incoming latents are summed with the softmax of their scores."""
        super().__init__()
        self.aggregation = _check_aggregation(aggregation, "NodeProcessor")
        if aggregation != "attention" and attention_hidden is not None:
            raise ValueError(f"NodeProcessor: attention_hidden belongs to aggregation='attention', not {aggregation!r}")
        self.node_processor = MLP(in_dim_node + in_dim_edge, in_dim_node, hidden_dim, hidden_layers, activation,
                                  initializer, norm_type)
        if aggregation == "attention":  # behind node_processor: it draws the random numbers it draws without the gate
            attention_hidden = 32 if attention_hidden is None else int(attention_hidden)
            if attention_hidden < 1:
                raise ValueError(f"NodeProcessor: attention_hidden {attention_hidden} must be positive")
            self.gate = MLP(in_dim_edge, 1, hidden_dim=attention_hidden, hidden_layers=1, activation="ReLU", norm_type=None)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor, u=None, batch=None):
        """MetaLayer node-model contract (models/GNN.py:95-104): MLP(cat[x, scatter_sum(e, col)]) + x."""
        dev = require_gpu_param(self.node_processor.model[0].weight, "NodeProcessor")
        back = x.device
        x, edge_attr = (t.to(device=dev, dtype=torch.float32) for t in (x, edge_attr))
        topo = get_topology(edge_index, x.size(0), dev)
        agg = self._aggregate(edge_attr, topo, topo.perm, topo.col32)
        out = _poison_if_deferred(topo, self.node_processor.forward_segments([(x, None), (agg, None)], residual=x))
        return out if back == dev else out.to(back)

    def _aggregate(self, edge_attr: Tensor, topo: GraphTopology, perm, dst_of_row, sums: Tensor | None = None) -> Tensor:
        """The [N, De] aggregate of ``edge_attr`` by ``self.aggregation``.  ``sums``: the per-destination SUMS where the edge
        launch's epilogue has formed them already (sum and mean; the max has no use for them)."""
        if self.aggregation == "max":  # the winners' rows are kept only under autograd
            return Fn.segment_max_csr(edge_attr, topo.rowptr, perm, dst_of_row, topo.num_nodes)
        if self.aggregation == "attention":  # one score per edge latent from the gate, then K21
            scores = self.edge_scores(edge_attr)
            return Fn.segment_softmax_csr(edge_attr, scores, topo.rowptr, perm, dst_of_row, topo.num_nodes)
        if sums is None:
            sums = Fn.scatter_sum_csr(edge_attr, topo.rowptr, perm, dst_of_row, topo.num_nodes)
        if self.aggregation == "mean":  # the sum machinery unchanged, then one launch over N rows: segment_mean_csr's bits
            return Fn.div_by_degree(sums, topo.rowptr, inplace=True)
        return sums

    def edge_scores(self, edge_attr: Tensor) -> Tensor:
        """[E] attention scores of the (updated) edge latents, in their row order (``aggregation="attention"`` only)."""
        return self.gate.forward_segments([(edge_attr, None)]).view(-1)

    def forward_sorted(self, x: Tensor, topo: GraphTopology, edge_attr: Tensor, agg: Tensor | None = None) -> Tensor:
        """``agg`` given: the per-destination sums already formed by the edge launch's epilogue."""
        agg = self._aggregate(edge_attr, topo, None, topo.dst_sorted, agg)
        return self.node_processor.forward_segments([(x, None), (agg, None)], residual=x)


# --------------------------------------------------------------------------- a4 MetaLayer glue
class MetaLayer(nn.Module):
    """The subset of ``torch_geometric.nn.MetaLayer`` the reference uses (models/GNN.py:24,
    :146-165, :215): ``edge_model`` then ``node_model``, no global model; attribute names are
    PyG's so ``state_dict`` keys match (``blocks.<i>.edge_model...``)."""

    def __init__(self, edge_model=None, node_model=None, global_model=None):
        super().__init__()
        if global_model is not None:
            raise NotImplementedError("global_model is not used by the reference and not implemented")
        self.edge_model = edge_model
        self.node_model = node_model
        self.global_model = None

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor | None = None, u=None, batch=None):
        dev = require_gpu_param(next(self.parameters()), "MetaLayer")
        back = x.device
        x = x.to(device=dev, dtype=torch.float32)
        edge_attr = edge_attr.to(device=dev, dtype=torch.float32)
        topo = get_topology(edge_index, x.size(0), dev)
        e_sorted = Fn.permute_rows(edge_attr, topo.perm, topo.inv_perm)
        x, e_sorted = self.forward_sorted(x, topo, e_sorted)
        edge_attr = Fn.permute_rows(e_sorted, topo.inv_perm, topo.perm)
        x, edge_attr = _poison_if_deferred(topo, x), _poison_if_deferred(topo, edge_attr)
        if back != dev:
            x, edge_attr = x.to(back), edge_attr.to(back)
        return x, edge_attr, u

    def forward_sorted(self, x: Tensor, topo: GraphTopology, edge_attr: Tensor, need_edges: bool = True):
        """``need_edges=False``: the caller drops the edge output, which may then come back as None (inference)."""
        agg = None
        if self.edge_model is not None:
            # let the edge launch form the node model's aggregate in its epilogue; with autograd on the
            # W-split Function returns both outputs and folds the aggregate's gradient (a gather) into e''s
            # (a max or attention aggregation has no epilogue inside the MFMA kernels: the edge launch stores e' - also in the
            # last block in inference - and K18 / K21 reduces it)
            if (FUSED_AGG and self.node_model is not None
                    and isinstance(self.edge_model, EdgeProcessor) and isinstance(self.node_model, NodeProcessor)
                    and self.node_model.aggregation not in ("max", "attention")):
                edge_attr, agg = self.edge_model.forward_sorted(x, topo, edge_attr, aggregate=True, need_edges=need_edges)
            else:
                edge_attr = self.edge_model.forward_sorted(x, topo, edge_attr)
        if self.node_model is not None:
            x = self.node_model.forward_sorted(x, topo, edge_attr, agg)
        return x, edge_attr


def build_GN_block(in_dim_node: int, in_dim_edge: int, hidden_dim_node: int = 128, hidden_dim_edge: int = 128,
                   hidden_layers_node: int = 2, hidden_layers_edge: int = 2, activation: str = "ReLU",
                   initializer: None | str = None, norm_type: None | str = "LayerNorm", aggregation: str = "sum",
                   attention_hidden: int | None = None):
    """models/GNN.py:110-165; ``aggregation`` and ``attention_hidden`` go to the block's ``NodeProcessor``."""
    _check_aggregation(aggregation, "build_GN_block")
    return MetaLayer(
        edge_model=EdgeProcessor(in_dim_node, in_dim_edge, hidden_dim_edge, hidden_layers_edge, activation,
                                 initializer, norm_type),
        node_model=NodeProcessor(in_dim_node, in_dim_edge, hidden_dim_node, hidden_layers_node, activation,
                                 initializer, norm_type, aggregation=aggregation, attention_hidden=attention_hidden),
    )


# --------------------------------------------------------------------------- a6 GraphProcessor
class GraphProcessor(nn.Module):
    def __init__(self, n_iterations: int, in_dim_node: int, in_dim_edge: int, hidden_dim_node: int = 128,
                 hidden_dim_edge: int = 128, hidden_layers_node: int = 2, hidden_layers_edge: int = 2,
                 activation: str = "ReLU", initializer: None | str = None, norm_type="LayerNorm", aggregation: str = "sum",
                 attention_hidden: int | None = None):
        """n_iterations GN blocks with unshared weights (models/GNN.py:168-211); ``aggregation`` (and ``attention_hidden``) is every
        block's."""
        super().__init__()
        self.aggregation = _check_aggregation(aggregation, "GraphProcessor")
        self.blocks = nn.ModuleList()
        for _ in range(n_iterations):
            self.blocks.append(build_GN_block(in_dim_node, in_dim_edge, hidden_dim_node, hidden_dim_edge,
                                              hidden_layers_node, hidden_layers_edge, activation, initializer,
                                              norm_type, aggregation=aggregation, attention_hidden=attention_hidden))

    def forward(self, x, edge_index, edge_attr):
        """models/GNN.py:213-216; ``edge_attr`` in and out in the caller's edge order."""
        if len(self.blocks) == 0:
            return x, edge_attr
        if getattr(self, "pools", None):
            raise ValueError("GraphProcessor.forward: top-K pooling (pool_ratio) changes the node and edge sets; call "
                             "GraphNet.forward / forward_device")
        dev = require_gpu_param(next(self.parameters()), "GraphProcessor")
        back = x.device
        x = x.to(device=dev, dtype=torch.float32)
        edge_attr = edge_attr.to(device=dev, dtype=torch.float32)
        topo = get_topology(edge_index, x.size(0), dev)
        x, e_sorted = self.forward_sorted(x, topo, Fn.permute_rows(edge_attr, topo.perm, topo.inv_perm))
        edge_attr = Fn.permute_rows(e_sorted, topo.inv_perm, topo.perm)
        x, edge_attr = _poison_if_deferred(topo, x), _poison_if_deferred(topo, edge_attr)
        if back != dev:
            x, edge_attr = x.to(back), edge_attr.to(back)
        return x, edge_attr

    def forward_sorted(self, x, topo: GraphTopology, edge_attr, need_edges: bool = True, graph_ptr: Tensor | None = None,
                       return_pooling: bool = False, compose_kept: bool = True):
        """``need_edges=False``: the caller drops the edge output; the last block may then return None for it.

        With pooling layers (``self.pools``, attached by ``GraphNet(pool_ratio=...)``): behind block k its ``TopKPool`` erases
        nodes, and the blocks after it run on the pooled rows and the pooled topology.  ``graph_ptr``: DEVICE int64 [G + 1]
        (None = all rows are one graph).  ``return_pooling=True``: ``(x, edge_attr, graph_ptr', kept)`` with the offsets of the
        pooled graphs and ``kept`` int32 [N'], the survivors' ORIGINAL rows (composed over the layers; None without pooling).

        Padded pooling layers (``TopKPool(padded=True)``) return everything at the input's sizes and read nothing back: ``x`` keeps
        its row count and ``edge_attr`` its edge count through all blocks, ``graph_ptr'`` ends at the device count N', and ``kept``
        [rows] holds -1 behind N'.  ``compose_kept=False``: the same tuple with ``kept`` None - the layers' lists are not composed (a
        read-out needs ``graph_ptr'`` alone)."""
        pools = getattr(self, "pools", None)
        last = len(self.blocks) - 1
        kept = None
        for k, block in enumerate(self.blocks):
            x, edge_attr = block.forward_sorted(x, topo, edge_attr, need_edges=need_edges or k < last)
            if pools and str(k) in pools:
                if graph_ptr is None:
                    graph_ptr = torch.arange(2, dtype=torch.int64, device=x.device) * x.size(0)  # [0, N], built on the device
                # behind the last block nothing reads the pooled edges: nodes only
                x, edge_attr, pooled_topo, graph_ptr, here = pools[str(k)].forward_sorted(x, topo, edge_attr, graph_ptr,
                                                                                          need_edges=need_edges or k < last)
                topo = pooled_topo if pooled_topo is not None else topo
                if return_pooling and compose_kept:
                    if kept is None:
                        kept = here
                    elif pools[str(k)].padded:  # -1 marks a slack entry: it must not index (it would wrap around to the last row)
                        kept = torch.where(here >= 0, kept[here.clamp(min=0).long()], here)
                    else:
                        kept = kept[here.long()]
        if return_pooling:
            return x, edge_attr, graph_ptr, kept
        return x, edge_attr


# --------------------------------------------------------------------------- K20 top-K node pooling
class TopKPool(nn.Module):
    """The pooling layer of the write-up's GN block (K20): ``score(v) = W2 relu(W1 h_v + b1) + b2`` from ``self.gate`` - an
    ``MLP(in_dim, 1, hidden_dim=hidden)`` with one hidden layer and no norm, on the fused-MLP kernels over all rows - then, per
    graph, the ``k = min(n, max(1, ceil(ratio n)))`` best nodes are kept in their old order and gated, ``h'_v = h_v tanh(score(v))``
    (``functional.topk_pool``).  One host read-back of the pooled sizes per call - none with ``padded=True``, the capacity-padded
    form whose outputs keep the input's sizes (a plain attribute: no parameter, no ``state_dict`` key)."""

    def __init__(self, in_dim: int, ratio: float, hidden: int = 32, padded: bool = False):
        super().__init__()
        self.ratio = native._check_ratio(ratio, "TopKPool")
        self.padded = bool(padded)
        self.gate = MLP(in_dim, 1, hidden_dim=int(hidden), hidden_layers=1, activation="ReLU", norm_type=None)

    def forward_sorted(self, x: Tensor, topo: GraphTopology, edge_attr: Tensor | None, graph_ptr: Tensor, need_edges: bool = True):
        """``(x', edge_attr', topo', graph_ptr', kept)`` on a prepared topology; ``edge_attr`` in its sorted edge order."""
        scores = self.gate.forward_segments([(x, None)]).view(-1)
        return Fn.topk_pool(x, scores, topo, graph_ptr, self.ratio, edge_attr if need_edges else None, need_edges=need_edges,
                            padded=self.padded)


def uses_node_pooling(model: nn.Module) -> bool:
    """True when ``model`` holds a ``TopKPool`` (of either form; ``pooling_reads_sizes_back`` tells them apart)."""
    return any(isinstance(m, TopKPool) for m in model.modules())


def pooling_reads_sizes_back(model: nn.Module) -> bool:
    """True when ``model`` holds a ``TopKPool`` that is not padded: its forward reads sizes back from the device, so it cannot be
    captured."""
    return any(isinstance(m, TopKPool) and not m.padded for m in model.modules())


def pooling_prevents_capture(model: nn.Module) -> bool:
    """True when no hipGraph capture takes ``model`` because of its top-K pooling: a sized pooling layer reads sizes back, and
    behind padded layers only a pooled read-out (a ``CombinedModel`` with ``readout`` other than ``"flatten"``) takes the graphs'
    rows through the device ``graph_ptr'`` - the flatten read-out and a bare ``GraphNet`` would have to narrow to N' on the host."""
    if not uses_node_pooling(model):
        return False
    return pooling_reads_sizes_back(model) or not (isinstance(model, CombinedModel) and model.pooled)


def _no_capture_with_pooling(model: nn.Module, who: str) -> None:
    if pooling_reads_sizes_back(model):
        raise ValueError(f"{who}: top-K node pooling (GraphNet(pool_ratio=...)) reads the pooled node and edge counts back from the "
                         f"device in every pooling layer, which a hipGraph capture cannot record; run this model eagerly, or build "
                         f"it with pool_padded=True")
    if pooling_prevents_capture(model):
        raise ValueError(f"{who}: padded top-K node pooling (GraphNet(pool_padded=True)) is captured under a pooled read-out alone "
                         f"(CombinedModel(readout='mean' / 'max' / 'sum' / 'hybrid' / 'attention')): the flatten read-out and a "
                         f"bare GraphNet narrow the rows to N' on the host")


# --------------------------------------------------------------------------- a7 GraphNet
class GraphNet(nn.Module):
    def __init__(self, **kwargs):
        """Encode-process-decode GraphNet; kwargs and defaults of models/GNN.py:223-295."""
        super().__init__()
        num_global_features = kwargs.get("num_global_features", 0)
        num_local_features = kwargs.get("num_local_features", 3)
        space_dim = kwargs.get("space_dim", 2)
        in_dim_node = num_local_features + num_global_features
        in_dim_edge = 1 + space_dim
        out_dim = kwargs.get("out_channels", 1)
        n_blocks = kwargs.get("n_blocks", 10)
        out_dim_node = kwargs.get("out_dim_node", 128)
        out_dim_edge = kwargs.get("out_dim_edge", 128)
        hidden_dim_node = kwargs.get("hidden_dim_node", 128)
        hidden_dim_edge = kwargs.get("hidden_dim_edge", 128)
        hidden_dim_decoder = kwargs.get("hidden_dim_decoder", 128)
        hidden_dim_processor_node = kwargs.get("hidden_dim_processor_node", 128)
        hidden_dim_processor_edge = kwargs.get("hidden_dim_processor_edge", 128)
        hidden_layers_node = kwargs.get("hidden_layers_node", 2)
        hidden_layers_edge = kwargs.get("hidden_layers_edge", 2)
        hidden_layers_decoder = kwargs.get("hidden_layers_decoder", 2)
        hidden_layers_processor_node = kwargs.get("hidden_layers_processor_node", 2)
        hidden_layers_processor_edge = kwargs.get("hidden_layers_processor_edge", 2)
        norm_type = kwargs.get("norm_type", "LayerNorm")
        activation = kwargs.get("activation", "ReLU")
        initializer = kwargs.get("initializer", None)
        # "sum" (the reference's code), "mean" (its write-up), "max" or "attention" (K21: a gate MLP per block scores the edge
        # latents); any other value is an error, never a silent sum
        aggregation = _check_aggregation(kwargs.get("aggregation", "sum"), "GraphNet")
        attention_hidden = kwargs.get("attention_hidden")  # with another mode the NodeProcessor raises
        # K20: top-K node pooling behind the GN blocks (the write-up's "Pooling(h(k))").  None: no pooling, no module, no keys.
        pool_ratio, pool_after, pool_hidden = kwargs.get("pool_ratio"), kwargs.get("pool_after"), kwargs.get("pool_hidden")
        # pool_padded: the capacity-padded pooling layers (no read-back, capturable).  No parameter, no key.
        pool_padded = bool(kwargs.get("pool_padded", False))
        if pool_ratio is None:
            if pool_after is not None or pool_hidden is not None or pool_padded:
                raise ValueError("GraphNet: pool_after / pool_hidden / pool_padded belong to pool_ratio, which is None")
        else:
            if pool_padded and norm_type == "BatchNorm1d":
                # batch statistics span ALL rows: the slack rows behind N' would enter them (LayerNorm is per row and unaffected)
                raise NotImplementedError("GraphNet(pool_padded=True): not with norm_type='BatchNorm1d'")
            pool_ratio = native._check_ratio(pool_ratio, "GraphNet(pool_ratio=...)")
            pool_after = list(range(n_blocks)) if pool_after is None else list(pool_after)
            if any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < n_blocks for i in pool_after) \
                    or len(set(pool_after)) != len(pool_after):
                raise ValueError(f"GraphNet: pool_after {pool_after!r} must hold distinct block indices in [0, {n_blocks})")
            pool_after = sorted(pool_after)
            pool_hidden = 32 if pool_hidden is None else int(pool_hidden)
            if pool_hidden < 1:
                raise ValueError(f"GraphNet: pool_hidden {pool_hidden} must be positive")

        self.name = "GraphNet"
        self.out_dim = out_dim
        self.space_dim = space_dim
        self.aggregation = aggregation

        self.node_encoder = MLP(in_dim_node, out_dim_node, hidden_dim_node, hidden_layers_node, activation=activation,
                                initializer=initializer, norm_type=norm_type)
        self.edge_encoder = MLP(in_dim_edge, out_dim_edge, hidden_dim_edge, hidden_layers_edge, activation=activation,
                                initializer=initializer, norm_type=norm_type)
        self.graph_processor = GraphProcessor(n_blocks, out_dim_node, out_dim_edge, hidden_dim_processor_node,
                                              hidden_dim_processor_edge, hidden_layers_processor_node,
                                              hidden_layers_processor_edge, activation=activation,
                                              initializer=initializer, norm_type=norm_type, aggregation=aggregation,
                                              attention_hidden=attention_hidden)
        self.node_decoder = MLP(out_dim_node, out_dim, hidden_dim_decoder, hidden_layers_decoder, norm_type=None)
        # the pools LAST: every other parameter draws the random numbers it draws without them (graph_processor.pools.<i>.gate.*)
        self.pool_ratio, self.pool_after = pool_ratio, tuple(pool_after) if pool_ratio is not None else ()
        self.pool_padded = pool_padded and bool(self.pool_after)
        if pool_ratio is not None and self.pool_after:
            self.graph_processor.pools = nn.ModuleDict({str(i): TopKPool(out_dim_node, pool_ratio, pool_hidden, padded=pool_padded)
                                                        for i in self.pool_after})

    @property
    def pooling(self) -> bool:
        """True when top-K pooling layers sit between the GN blocks: the output then has fewer rows than the input."""
        return bool(self.pool_after)

    def pooled_nodes(self, n: int) -> int:
        """Rows the output holds for ONE graph of ``n`` nodes: ``k = min(n, max(1, ceil(ratio n)))`` applied once per pooling layer."""
        n = int(n)
        for _ in self.pool_after:
            n = native.topk_keep_count(self.pool_ratio, n)
        return n

    def forward_device(self, x: Tensor, pos: Tensor, topo: GraphTopology, graph_ptr: Tensor | None = None,
                       return_pooling: bool = False, compose_kept: bool = True):
        """GraphNet.forward on device tensors with a prepared topology (models/GNN.py:297-309).  ``graph_ptr``: DEVICE int64
        [G + 1] offsets of the graphs, read by the pooling layers alone (None = one graph; rows of no graph are erased by the first
        pooling layer).  ``return_pooling=True``: ``(out, graph_ptr', kept)`` - the offsets of the rows of ``out`` (``graph_ptr``
        itself without pooling) and the ORIGINAL rows of the survivors, int32 ascending (None without pooling).  With pooling every
        pooling layer reads two sizes back from the device (one host synchronisation each) - unless the layers are padded
        (``pool_padded=True``): then nothing is read back, ``out`` keeps all ``rows`` rows, of which those at or behind
        ``graph_ptr'[-1]`` = N' are unspecified, and ``kept`` int32 [rows] holds -1 behind N'.  ``compose_kept=False``:
        ``(out, graph_ptr', None)`` - ``kept`` is not composed over the layers (what a read-out needs)."""
        out = self.node_encoder.forward_segments([(x.view(x.size(0), -1), None)])         # :305
        # :299-302 + :306: K6 as the prologue of the edge encoder's launch where a kernel offers it (inference, large batches)
        edge_attr = self.edge_encoder.forward_edge_features(pos, topo.src_sorted, topo.dst_sorted)
        if edge_attr is None:
            edge_attr = Fn.edge_features(pos, topo.src_sorted, topo.dst_sorted)           # :299-302 (K6)
            edge_attr = self.edge_encoder.forward_segments([(edge_attr, None)])           # :306
        kept = None
        if self.pooling:
            # the sized layers compose ``kept`` as they always did; behind padded layers only a caller that takes it pays for it
            compose = compose_kept and (return_pooling or not self.pool_padded)
            out, _, graph_ptr, kept = self.graph_processor.forward_sorted(out, topo, edge_attr, need_edges=not DROP_DEAD_EDGE_STORE,
                                                                          graph_ptr=graph_ptr, return_pooling=True, compose_kept=compose)
        else:
            out, _ = self.graph_processor.forward_sorted(out, topo, edge_attr, need_edges=not DROP_DEAD_EDGE_STORE)  # :307
        out = self.node_decoder.forward_segments([(out, None)])                           # :308
        # validation not read back yet: a bad edge_index must not yield a plausible result (the ORIGINAL topology's flags)
        out = _poison_if_deferred(topo, out)
        return (out, graph_ptr, kept) if return_pooling else out

    @torch.no_grad()
    def edge_attention_weights(self, x: Tensor, pos: Tensor, edge_index: Tensor) -> list[Tensor]:
        """``aggregation="attention"``: one ``alpha`` [E] per GN block, in the caller's edge order - the weight each edge's latent
        has in its destination's aggregate; it sums to 1 over the incoming edges of every node that has any."""
        if self.aggregation != "attention":
            raise ValueError(f"GraphNet.edge_attention_weights: aggregation is {self.aggregation!r}, not 'attention'")
        if self.pooling:
            raise ValueError("GraphNet.edge_attention_weights: top-K pooling changes the edge set between the blocks")
        dev = require_gpu_param(self.node_encoder.model[0].weight, "GraphNet")
        back = x.device
        x = x.to(device=dev, dtype=torch.float32)
        pos = pos.to(device=dev, dtype=torch.float32)
        topo = get_topology(edge_index, x.size(0), dev)
        h = self.node_encoder.forward_segments([(x.view(x.size(0), -1), None)])
        e = Fn.edge_features(pos, topo.src_sorted, topo.dst_sorted)
        e = self.edge_encoder.forward_segments([(e, None)])
        weights = []
        for block in self.graph_processor.blocks:
            e = block.edge_model.forward_sorted(h, topo, e)
            node = block.node_model
            scores = node.edge_scores(e)
            agg, saved = native.segment_softmax_csr(e, scores, topo.rowptr, None, topo.num_nodes)
            alpha = native.segment_softmax_weights(scores, saved, topo.dst_sorted)
            alpha = alpha[topo.inv_perm.long()]  # sorted position -> the caller's edge order
            if topo.deferred:  # flags not read back yet: a bad edge_index must not yield plausible weights
                alpha = torch.where(topo.status.any(), torch.full_like(alpha, float("nan")), alpha)
            weights.append(alpha)
            h = node.node_processor.forward_segments([(h, None), (agg, None)], residual=h)
        return [w if back == dev else w.to(back) for w in weights]

    def forward(self, x, pos, edge_index):
        dev = require_gpu_param(self.node_encoder.model[0].weight, "GraphNet")
        back = x.device
        x = x.to(device=dev, dtype=torch.float32)
        pos = pos.to(device=dev, dtype=torch.float32)
        topo = get_topology(edge_index, x.size(0), dev)
        if self.pool_padded:  # the public shape is the sized mode's: ONE read of N' narrows the padded rows
            out, graph_ptr, _ = self.forward_device(x, pos, topo, return_pooling=True, compose_kept=False)
            out = out[:int(graph_ptr[-1].item())]
        else:
            out = self.forward_device(x, pos, topo)
        return out if back == dev else out.to(back)


def _has_batchnorm(model: nn.Module) -> bool:
    """Batch statistics span ALL rows of a launch: the dummy rows of a padded feed would enter them."""
    return any(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in model.modules())


def _same_topology(a: Tensor, b: Tensor) -> bool:
    return a is b or (a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and bool(torch.equal(a, b)))


class FixedGraphFeed:
    """The input buffers of a hipGraph captured for ONE topology: ``x`` / ``pos`` of the sample's shape, its edge list on the
    device with the topology built from it (the build's host sync happens here, outside the capture), and ``graph_ptr`` = [0, N]
    (``_whole``) for the pooling layers and a pooled read-out.  A call is two copies."""

    edge_capacity = node_capacity = None

    def __init__(self, x: Tensor, pos: Tensor, edge_index: Tensor, device):
        self.x = x.to(device=device, dtype=torch.float32).clone()
        self.pos = pos.to(device=device, dtype=torch.float32).clone()
        self.edge_index, self._given = edge_index.to(device), edge_index
        self.num_nodes = int(x.size(0))
        self.topo = get_topology(self.edge_index, self.num_nodes, device)
        self.graph_ptr = self._whole = torch.tensor([0, self.num_nodes], dtype=torch.int64, device=device)

    def matches(self, sample) -> bool:
        x, pos, edge_index = sample
        return x.shape == self.x.shape and pos.shape == self.pos.shape and _same_topology(edge_index, self._given)

    def __call__(self, x: Tensor, pos: Tensor | None = None, edge_index: Tensor | None = None) -> None:
        self.x.copy_(x, non_blocking=True)
        if pos is not None:
            self.pos.copy_(pos, non_blocking=True)

    def check(self, status: Tensor | None) -> None:
        pass


class PaddedGraphFeed:
    """The fixed input buffers of a hipGraph captured for ANY single graph that fits them (superpixel graphs: a new region adjacency
    per image, utils/image_to_graph/image_to_graph_superpixel.py:31-66, and with ``node_capacity`` another segment count too), and
    the copies that fill them.  Pure torch: it runs on any device.

    With ``C = edge_capacity``, ``D = dummies = max(1, ceil(C / 8))`` and ``S`` node slots (``node_capacity``, or the sample's node
    count when that is None: every graph then has that many nodes): ``x`` / ``pos`` hold ``rows = max(S + D, min_rows)`` rows - a
    sample's n rows, isolated zero rows up to S, D zero dummy rows that are never written; ``edge_index`` [2, C] holds a sample's
    edges and, behind them, self-loops of the dummies, spread round-robin (at most 8 each: ONE dummy would be a hub of hundreds of
    rows that the per-destination kernels walk serially, 0.95 ms per step against 0.6).  Dummies only talk to dummies, so whatever
    reads rows ``[0, n)`` alone sees the plain graph's result, bit for bit, and the rest gets exact zero gradients.
    ``graph_ptr`` = [0, n] is a pooled read-out's offsets; ``valid_nodes`` is its second entry, the SAME storage, which a call
    under ``node_capacity`` rewrites in front of the replay.  The range flag is sticky: a call sets it when a DEVICE edge list
    names a row at or behind n (ids in ``[n, rows)`` pass the topology build's range check but are not nodes of this graph;
    reading them here would synchronise), and only ``check`` clears it.  A HOST edge list is checked in the call itself.

    ``keep_missing``: in the ``edge_capacity``-only form a call may pass ``pos=None`` / ``edge_index=None`` and keep the buffer's
    contents (``CapturedForward``)."""

    def __init__(self, x: Tensor, pos: Tensor, edge_index: Tensor, edge_capacity: int, node_capacity: int | None = None, *,
                 device, min_rows: int = 0, keep_missing: bool = False, who: str = "PaddedGraphFeed"):
        self.who, self.keep_missing = who, keep_missing
        self.edge_capacity, self.node_capacity = C, M = int(edge_capacity), node_capacity
        self.num_nodes = self._filled = n = int(x.size(0))  # of the sample fed last; rows of x / pos that hold a sample
        self._require_fit(n, int(edge_index.size(1)))
        self.dummies = dummies = max(1, (C + 7) // 8)
        slots = n if M is None else M
        self.rows = max(slots + dummies, min_rows)
        self.x = torch.zeros(self.rows, *x.shape[1:], dtype=torch.float32, device=device)
        self.pos = torch.zeros(self.rows, *pos.shape[1:], dtype=torch.float32, device=device)
        self._tail = slots + torch.arange(C, dtype=torch.int64, device=device) % dummies  # slot k's dummy self-loop
        self.edge_index = self._tail.repeat(2, 1)
        self.graph_ptr = torch.tensor([0, n], dtype=torch.int64, device=device)
        self.valid_nodes = self.graph_ptr[1]
        self._range_flag = torch.zeros((), dtype=torch.bool, device=device)
        self.x[:n].copy_(x)
        self.pos[:n].copy_(pos)
        self.edge_index[:, :edge_index.size(1)].copy_(edge_index)

    def _nodes_fit(self, n: int) -> bool:
        return n == self.num_nodes if self.node_capacity is None else n <= self.node_capacity

    def matches(self, sample) -> bool:
        x, pos, edge_index = sample
        return (self._nodes_fit(x.size(0)) and x.shape[1:] == self.x.shape[1:] and pos.shape[1:] == self.pos.shape[1:]
                and edge_index.dim() == 2 and edge_index.size(1) <= self.edge_capacity)

    def _require_fit(self, n: int, e: int) -> None:
        if not self._nodes_fit(n) or e > self.edge_capacity:
            nodes = self.num_nodes if self.node_capacity is None else f"at most {self.node_capacity}"
            raise ValueError(f"{self.who}: a sample with {n} nodes / {e} edges does not fit the captured {nodes} nodes / "
                             f"at most {self.edge_capacity} edges")

    def __call__(self, x: Tensor, pos: Tensor | None, edge_index: Tensor | None) -> None:
        if (pos is None or edge_index is None) and not (self.keep_missing and self.node_capacity is None):
            form = "" if self.node_capacity is None else "(node_capacity=...)"
            raise ValueError(f"{self.who}{form}: every call needs x, pos and edge_index")
        n, e = int(x.size(0)), 0 if edge_index is None else int(edge_index.size(1))
        self._require_fit(n, e)
        if self.node_capacity is not None:
            if n < self._filled:  # a smaller graph after a larger one: its slots become isolated zero nodes again
                self.x[n:self._filled].zero_()
                self.pos[n:self._filled].zero_()
            self.num_nodes = self._filled = n
            self.valid_nodes.fill_(n)
        self.x[:n].copy_(x, non_blocking=True)
        if pos is not None:
            self.pos[:n].copy_(pos, non_blocking=True)
        if edge_index is None:
            return
        if e and not edge_index.is_cuda:
            if int(edge_index.max()) >= n or int(edge_index.min()) < 0:
                raise IndexError(f"edge_index has node ids outside [0, {n})")
        elif e:
            self._range_flag |= (edge_index >= n).any()
        self.edge_index[:, :e].copy_(edge_index, non_blocking=True)
        self.edge_index[:, e:].copy_(self._tail[e:])

    def check(self, status: Tensor | None) -> None:
        """One host sync for the sticky flag and ``status`` (the flags of the LAST replayed topology build); clears the sticky
        flag and raises the IndexError of models/GNN.py:18-20 when either is set (the output of such a replay is NaN)."""
        if bool((self._range_flag if status is None else self._range_flag | status.any()).item()):
            self._range_flag.zero_()
            raise IndexError(f"edge_index has node ids outside [0, {self.num_nodes})")


class RaggedBatchFeed:
    """The fixed input buffers of a hipGraph captured over RAGGED mini-batches (superpixel batches: another region adjacency and
    other node counts in every batch) and the ONE launch that fills them from a collated ``synthetic.GraphBatch``
    (``native.pad_graph_batch``; the host offsets and labels travel in the kernel arguments, so a call copies nothing else).

    With ``M = node_capacity``, ``C = edge_capacity`` and ``rows, D = native.ragged_batch_layout(M, C)``: ``x`` / ``pos`` hold the
    batch's N rows, zero slack rows ``[N, M)`` that belong to no graph, and D zero dummy rows that are never written;
    ``edge_index`` [2, C] holds the batch's E edges and, behind them, self-loops of the dummies; ``graph_ptr`` [G + 1] and
    ``labels`` [G] are int64.  ``flag`` is sticky: the feed sets it when an edge leaves its own graph's node range (another
    graph, a slack or dummy row, a negative id), and only ``check`` clears it.  G is fixed."""

    def __init__(self, batch, edge_capacity: int, node_capacity: int, device, with_labels: bool, who: str = "RaggedBatchFeed"):
        self.who = who
        self.num_graphs = G = int(batch.num_graphs)
        self.edge_capacity, self.node_capacity = C, M = int(edge_capacity), int(node_capacity)
        if G > native.PAD_BATCH_MAX_GRAPHS:
            raise ValueError(f"{who}: {G} graphs, the feed launch takes at most {native.PAD_BATCH_MAX_GRAPHS}")
        self.feature_shapes = (tuple(batch.x.shape[1:]), tuple(batch.pos.shape[1:]))
        self._require_fit(batch)
        self.rows, self.dummies = native.ragged_batch_layout(M, C)
        self.x = torch.zeros(self.rows, *self.feature_shapes[0], dtype=torch.float32, device=device)
        self.pos = torch.zeros(self.rows, *self.feature_shapes[1], dtype=torch.float32, device=device)
        self.edge_index = torch.zeros(2, C, dtype=torch.int64, device=device)
        self.graph_ptr = torch.zeros(G + 1, dtype=torch.int64, device=device)
        self.labels = torch.zeros(G, dtype=torch.int64, device=device) if with_labels else None
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.num_nodes = 0  # of the batch fed last (the IndexError's message)

    def matches(self, batch) -> bool:
        return (int(batch.num_graphs) == self.num_graphs and batch.x.size(0) <= self.node_capacity
                and batch.edge_index.dim() == 2 and batch.edge_index.size(1) <= self.edge_capacity
                and (tuple(batch.x.shape[1:]), tuple(batch.pos.shape[1:])) == self.feature_shapes)

    def _require_fit(self, batch) -> None:
        if not self.matches(batch):
            raise ValueError(f"{self.who}: a batch of {int(batch.num_graphs)} graphs / {batch.x.size(0)} nodes / "
                             f"{batch.edge_index.size(1)} edges with features {tuple(batch.x.shape[1:])} / {tuple(batch.pos.shape[1:])} "
                             f"does not fit the captured {self.num_graphs} graphs / {self.node_capacity} nodes / "
                             f"{self.edge_capacity} edges with features {self.feature_shapes[0]} / {self.feature_shapes[1]}")

    def __call__(self, batch, labels=None) -> None:
        self._require_fit(batch)
        if (labels is None) != (self.labels is None):
            raise ValueError(f"{self.who}: labels are {'not ' if self.labels is None else ''}part of this capture")
        dev = self.x.device
        x = batch.x.to(device=dev, dtype=torch.float32, non_blocking=True)
        pos = batch.pos.to(device=dev, dtype=torch.float32, non_blocking=True)
        ei = batch.edge_index.to(device=dev, dtype=torch.int64, non_blocking=True)
        by_value = labels
        if isinstance(labels, Tensor) and labels.is_cuda:  # device labels: reading them would synchronise; one small copy instead
            self.labels.copy_(labels.reshape(-1), non_blocking=True)
            by_value = None
        native.pad_graph_batch(x, pos, ei, batch.graph_ptr, batch.edge_ptr, by_value, self.node_capacity, self.edge_capacity,
                               self.x, self.pos, self.edge_index, self.graph_ptr, self.labels if by_value is not None else None,
                               self.flag)
        self.num_nodes = int(batch.x.size(0))

    def check(self, status: Tensor | None) -> None:
        """One host sync for the sticky flag and ``status`` (the flags of the LAST replayed topology build); clears the sticky
        flag and raises the IndexError of models/GNN.py:18-20 when either is set."""
        flags = self.flag if status is None else torch.cat([self.flag, status.reshape(-1).to(torch.int32)])
        if any(flags.tolist()):
            self.flag.zero_()
            raise IndexError(f"edge_index has node ids outside their graph's node range (batch of {self.num_nodes} nodes)")


def graph_logits(mod: nn.Module, feed):
    """``(logits, status)`` of the single graph in a ``FixedGraphFeed`` or ``PaddedGraphFeed``, for ``mod`` a ``CombinedModel`` or a
    bare ``GraphNet`` (whose "logits" are its node rows).  Over a padded feed the topology is built HERE, from whatever edge list
    the buffer holds (deferred validation: device flags, no host sync, never the cache), so it is part of whatever records this
    call; ``status`` are that build's flags, for the feed's ``check`` (None over a fixed feed, whose topology was validated)."""
    if feed.edge_capacity is None:
        topo, status = feed.topo, None
    else:
        topo = GraphTopology(feed.edge_index, feed.rows, device=feed.x.device, validate="deferred")
        status = topo.status
    gnet = getattr(mod, "graph_net", mod)
    pooled = bool(getattr(mod, "pooled", False))  # a read-out that takes the graph's rows through a device graph_ptr
    if pooled and gnet.pooling:  # padded top-K pooling: the first layer erases the slots and the dummies with the rows of no
        # graph, and the read-out takes the POOLED graph's rows [0, N')
        y, ptr, _ = gnet.forward_device(feed.x, feed.pos, topo, graph_ptr=feed.graph_ptr, return_pooling=True, compose_kept=False)
        return mod.readout_logits(y, ptr)[0], status
    y = gnet.forward_device(feed.x, feed.pos, topo)
    if pooled:  # rows [0, valid_nodes): the slots behind them and the dummies are outside the graph
        return mod.readout_logits(y, feed.graph_ptr)[0], status
    if feed.node_capacity is not None:
        return mod.classifier(masked_readout_rows(y, mod.num_nodes, feed.valid_nodes).flatten()), status
    y = y[:feed.num_nodes]
    return (y if gnet is mod else mod.classifier(y.flatten())), status


def ragged_batch_logits(mod: nn.Module, feed: RaggedBatchFeed):
    """``(logits [G, classes], status)`` of the mini-batch in a ``RaggedBatchFeed``: ``graph_logits``' padded form for G graphs."""
    topo = GraphTopology(feed.edge_index, feed.rows, device=feed.x.device, validate="deferred")
    return mod.forward_batched_device(feed.x, feed.pos, topo, graph_ptr=feed.graph_ptr), topo.status


def flatten_readout_rows(model: nn.Module, node_capacity: int | None, pooled: bool) -> int:
    """``min_rows`` of a ``PaddedGraphFeed`` for ``model``: the flatten read-out of the ``node_capacity`` form takes rows
    ``[0, model.num_nodes)`` whatever the capacity is."""
    return int(model.num_nodes) if node_capacity is not None and not pooled and hasattr(model, "num_nodes") else 0


class _Captured:
    """A feed, a closure over the feed's buffers, and the hipGraph that recorded the closure: what every capture class is.
    ``matches`` and ``check`` are the feed's, and so is every attribute the capture does not set itself: ``x`` / ``pos`` /
    ``edge_index`` (the very tensors the graph reads), ``num_nodes``, ``valid_nodes``, the capacities, ``num_graphs``."""

    def __getattr__(self, name):
        if name == "feed":
            raise AttributeError(name)
        return getattr(self.feed, name)

    def _record(self, device, fn, warmups: int, warm=None, capture_error_mode: str = "global"):
        """Runs ``warm`` (default: ``fn``) ``warmups`` times on a side stream - kernel attributes, allocator pools, lazily built CSR
        forms - then records ``fn`` into ``self.graph`` and returns what the recorded call returned.

        **Who keeps a recorded buffer alive.**  A hipGraph records ADDRESSES.  A tensor that ``fn`` reads and that was allocated
        outside the recording must therefore live as long as the graph does, or its memory goes back to the allocator, the next
        small allocation lands on it, and every later replay reads those bytes.  The rule: the capture object owns the closure
        it recorded (``self._recorded``), and through it everything the closure holds - the feed, the model, a caller's
        ``forward=`` and whatever THAT closes over.  No caller and no subclass has to keep anything alive by hand.  (Tensors
        allocated inside the recording live in the graph's own pool.)"""
        self._recorded = fn
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(warmups):
                (warm or fn)()
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode=capture_error_mode):
            return fn()

    def matches(self, *sample) -> bool:
        return self.feed.matches(*sample)

    def check(self) -> None:
        """One host sync: the feed's sticky flag and the flags of the last replayed topology build; raises the IndexError of
        models/GNN.py:18-20 for node ids outside the graph."""
        self.feed.check(self._status)


class CapturedForward(_Captured):
    """A GraphNet / CombinedModel forward captured into a hipGraph.  Inference only (no autograd through a replay).

    The reference's training and inference loops run one small graph per call (main.py:60, utils/inference.py:59); at ~1000 nodes
    the ~30 kernel launches of a forward are launch-bound (about 1 ms eager).  A call copies its arguments into the feed's
    buffers, one ``hipGraphLaunch`` runs every kernel, and ``out`` is the result buffer (rewritten by the next call).

    The feed decides what a call may bring: ONE topology (``FixedGraphFeed``: pixel / patch graphs, the same edge list for every
    image of a size, optimized.py:42-47; the edge list of a call is not read); with ``edge_capacity``, ANY edge list over the
    sample's node count; with ``node_capacity`` as well, for a ``CombinedModel`` with ``ragged_readout``, any graph that fits both
    (``PaddedGraphFeed``).  Over a padded feed the read-out follows ``graph_logits``: the flatten read-out takes rows
    ``[0, num_nodes)`` and zeroes those at or behind the device count ``valid_nodes`` - the rule of
    ``CombinedModel.ragged_readout`` - and a pooled one (``readout="mean"`` ...) pools rows ``[0, valid_nodes)``."""

    def __init__(self, model: nn.Module, x: Tensor, pos: Tensor, edge_index: Tensor, edge_capacity: int | None = None,
                 node_capacity: int | None = None):
        who = "CapturedForward"
        _no_capture_with_pooling(model, who)
        dev = require_gpu_param(next(model.parameters()), who)
        combined = isinstance(model, CombinedModel)
        if node_capacity is not None:
            if edge_capacity is None:
                raise ValueError(f"{who}: node_capacity requires edge_capacity")
            if not (combined and model.ragged_readout):
                raise TypeError(f"{who}(node_capacity=...): a CombinedModel with ragged_readout = True expected")
        if edge_capacity is None:
            feed = FixedGraphFeed(x, pos, edge_index, dev)
        else:
            if model.training and _has_batchnorm(model):  # eval mode normalises row by row
                raise NotImplementedError(f"{who}(edge_capacity=...): a BatchNorm model must be in eval() mode")
            feed = PaddedGraphFeed(x, pos, edge_index, edge_capacity, node_capacity, device=dev, keep_missing=True, who=who,
                                   min_rows=flatten_readout_rows(model, node_capacity, combined and model.pooled))
        self._init(model, feed, graph_logits)

    def _init(self, model: nn.Module, feed, logits) -> None:
        self.model, self.feed, self.device = model, feed, feed.x.device
        with torch.no_grad():
            self.out, self._status = self._record(self.device, lambda: logits(model, feed), 2)

    def __call__(self, x: Tensor, pos: Tensor | None = None, edge_index: Tensor | None = None) -> Tensor:
        self.feed(x, pos, edge_index)
        self.graph.replay()
        return self.out


class CapturedRaggedBatchForward(CapturedForward):
    """``CombinedModel.forward_batched(graph_ptr=...)`` for ANY mini-batch of G graphs with at most ``node_capacity`` nodes and
    ``edge_capacity`` edges in all: ``CapturedForward`` over a ``RaggedBatchFeed`` and ``ragged_batch_logits``.  A call is the feed
    launch and the replay.  Slack and dummy rows only talk to dummies and belong to no graph, so the logits [G, classes] are those
    of the eager call.  G is fixed per capture; a call with a batch that does not ``matches`` raises ValueError."""

    def __init__(self, model: nn.Module, batch, edge_capacity: int, node_capacity: int):
        who = "CapturedRaggedBatchForward"
        if not isinstance(model, CombinedModel):
            raise TypeError(f"{who}: a CombinedModel expected")
        _no_capture_with_pooling(model, who)
        dev = require_gpu_param(next(model.parameters()), who)
        if model.training and _has_batchnorm(model):  # eval mode normalises row by row
            raise NotImplementedError(f"{who}: a BatchNorm model must be in eval() mode")
        feed = RaggedBatchFeed(batch, edge_capacity, node_capacity, dev, with_labels=False, who=who)
        feed(batch)
        self._init(model, feed, ragged_batch_logits)

    def __call__(self, batch) -> Tensor:
        self.feed(batch)
        self.graph.replay()
        return self.out


# --------------------------------------------------------------------------- a8 read-out
def ragged_readout_rows(y: Tensor, num_nodes: int) -> Tensor:
    """The read-out rule for a graph whose node count is not ``num_nodes`` (``forward_batched(graph_ptr=...)``'s): the
    first ``num_nodes`` rows of ``y`` [N, out_dim], zero rows behind a smaller graph.  Differentiable."""
    n = y.size(0)
    if n >= num_nodes:
        return y[:num_nodes]
    return torch.cat([y, y.new_zeros(num_nodes - n, *y.shape[1:])])


def masked_readout_rows(y: Tensor, num_nodes: int, valid_nodes: Tensor) -> Tensor:
    """The same rule on fixed shapes, for a hipGraph: rows ``[0, num_nodes)`` of a padded ``y``, those at or behind the
    DEVICE count ``valid_nodes`` replaced by zeros (a select, not a product: no ``-0.0`` from a negative row)."""
    keep = torch.arange(num_nodes, device=y.device) < valid_nodes
    return torch.where(keep[:, None], y[:num_nodes], y.new_zeros(()))


class LinearClassifier(nn.Module):
    def __init__(self, in_features=128 * 128, classes=2):
        """models/GNN.py:312-325; three small dense layers left to PyTorch-ROCm."""
        super().__init__()
        self.fc1 = nn.Linear(in_features=in_features, out_features=128)
        self.fc2 = nn.Linear(in_features=128, out_features=32)
        self.fc3 = nn.Linear(in_features=32, out_features=classes)
        self.relu = nn.ReLU()

    def forward(self, x):
        if (READOUT_HIP and x.dim() == 1 and x.is_cuda and x.dtype == torch.float32 and self.fc1.weight.is_cuda
                and self.fc1.out_features <= native.READOUT_MAX_HIDDEN and self.fc2.out_features <= native.READOUT_MAX_HIDDEN
                and self.fc3.out_features <= native.READOUT_MAX_CLASSES):
            # ONE graph (the reference's loops): the three matrix-vector products in one launch each way (csrc/readout.hip)
            return Fn.readout(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.fc3.weight, self.fc3.bias)
        x = self.relu(self.fc1(x))
        x = self.relu(self.fc2(x))
        return self.fc3(x)


class CombinedModel(nn.Module):
    READOUTS = ("flatten", "mean", "max", "sum", "hybrid", "attention")

    def __init__(self, graph_net: GraphNet | None = None, num_nodes: int = 128 * 128, classes: int = 2, *, readout: str = "flatten",
                 gate_hidden: int | None = None):
        """models/GNN.py:327-332.  ``readout="flatten"`` is the reference's model: ``fc1`` over the ``num_nodes * out_dim`` flattened
        node outputs.  ``"mean"`` / ``"max"`` / ``"sum"`` / ``"hybrid"``: a global pooling read-out (the one the reference's write-up
        describes; K17) hands ONE vector per graph - ``out_dim`` wide, ``3 * out_dim`` for ``hybrid`` = [mean | max | sum] - to the
        same three-layer classifier.  It is permutation invariant and defined for every node count; ``num_nodes`` is kept but
        sizes nothing.  Same ``state_dict`` keys either way; ``readout`` is not stored in it.

        ``"attention"`` (K19): the write-up's attention read-out.  A gate ``score(v) = W2 relu(W1 h_v + b1) + b2`` - ``self.gate``,
        an ``MLP(out_dim, 1, hidden_dim=gate_hidden)`` with one hidden layer of ``gate_hidden`` (32 by default) units and no norm
        - scores every node, and the graph's vector is the sum of its node outputs weighted by the softmax of the scores over the
        graph: ``out_dim`` wide, permutation invariant, defined for every node count.  The gate is built AFTER the classifier, so
        under one seed every other parameter equals the ``"mean"`` model's; its keys ``gate.model.0.*`` / ``gate.model.2.*`` exist for
        this read-out alone, and ``gate_hidden`` with another read-out is a ValueError.  A checkpoint of another pooled read-out
        loads with ``load_state_dict(..., strict=False)``: the gate then stays at its initialisation."""
        super().__init__()
        if readout not in self.READOUTS:
            raise ValueError(f"CombinedModel: readout {readout!r} is not one of {self.READOUTS}")
        if gate_hidden is not None and readout != "attention":
            raise ValueError(f"CombinedModel: gate_hidden belongs to readout='attention', not to {readout!r}")
        self.graph_net = graph_net if graph_net is not None else GraphNet()
        self.num_nodes = num_nodes
        self.readout = readout
        if readout == "flatten":
            in_features = num_nodes * self.graph_net.out_dim
        else:
            in_features = (3 if readout == "hybrid" else 1) * self.graph_net.out_dim
        self.classifier = LinearClassifier(in_features=in_features, classes=classes)
        if readout == "attention":  # after the classifier: the other parameters draw the random numbers they draw without it
            self.gate = MLP(self.graph_net.out_dim, 1, hidden_dim=32 if gate_hidden is None else int(gate_hidden), hidden_layers=1,
                            activation="ReLU", norm_type=None)
        # True: ``forward`` accepts a graph of any node count N.  On the flatten model (off by default; a plain attribute, not a
        # constructor argument and not in the state_dict) it feeds fc1 rows [0, min(N, num_nodes)) of the GraphNet output, the rest
        # of the vector zero (forward_batched(graph_ptr=...)'s rule; the reference's read-out is only defined for
        # N == num_nodes).  A pooled model accepts any node count by construction and answers True.
        self.ragged_readout = readout != "flatten"
        self.to(next(self.graph_net.parameters()).device)

    @property
    def pooled(self) -> bool:
        return self.readout != "flatten"

    def readout_logits(self, y: Tensor, graph_ptr: Tensor | None, num_graphs: int | None = None) -> Tensor:
        """The read-out behind the GraphNet: logits [G, classes] from the node outputs ``y`` [rows, out_dim] and a DEVICE int64
        ``graph_ptr`` [G + 1] (``None`` on the flatten model: ``num_graphs`` graphs of exactly ``num_nodes`` rows).  Rows outside
        the graphs are ignored and get zero gradient.  No host synchronisation: every caller - ``forward``, the batched forms, the
        captured forwards and steps - comes through here with a pooled model."""
        fc1, fc2, fc3 = self.classifier.fc1, self.classifier.fc2, self.classifier.fc3
        od = self.graph_net.out_dim
        gp = graph_ptr
        if gp is not None:
            num_graphs = gp.numel() - 1
        if self.pooled:
            if self.readout == "attention":  # the gate scores ALL rows; rows of no graph get zero score gradient from K19
                feats = Fn.graph_attention_pool(y, self.gate.forward_segments([(y, None)]).view(-1), gp)  # [G, out_dim]
            else:
                feats = Fn.graph_pool(y, gp, self.readout)  # [G, F]
            if num_graphs == 1:
                return self.classifier(feats[0]).unsqueeze(0)  # the single-graph launch (csrc/readout.hip)
            if READOUT_HIP and native.readout_batched_supported(num_graphs, feats.size(1), fc1.out_features, fc2.out_features,
                                                                fc3.out_features):
                # K13 over the pooled matrix: G "graphs" of one node with F outputs each
                return Fn.readout_batched(feats, None, num_graphs, 1, fc1.weight, fc1.bias, fc2.weight, fc2.bias, fc3.weight, fc3.bias)
            return self.classifier(feats)
        if (READOUT_HIP and num_graphs >= 1 and y.dtype == torch.float32 and fc1.in_features == self.num_nodes * od
                and native.readout_batched_supported(num_graphs, fc1.in_features, fc1.out_features, fc2.out_features,
                                                     fc3.out_features)):
            # the gather rule below fused into fc1's operand load, fc1 on MFMA, fc2 / fc3 from LDS (csrc/readout_batched.hip);
            # a shape the library does not take stays on the torch path
            return Fn.readout_batched(y, gp, num_graphs, self.num_nodes, fc1.weight, fc1.bias, fc2.weight, fc2.bias,
                                      fc3.weight, fc3.bias)
        if gp is None:
            feats = y.view(num_graphs, -1)
        else:
            start, size = gp[:-1], gp[1:] - gp[:-1]
            k = torch.arange(self.num_nodes, device=y.device)
            valid = k[None, :] < size[:, None]                                   # [G, num_nodes]
            rows = (start[:, None] + k[None, :]).clamp_(max=max(y.size(0) - 1, 0))
            feats = (y[rows] * valid[..., None]).reshape(gp.numel() - 1, self.num_nodes * od)
        return self.classifier(feats)

    def attention_weights(self, x, pos=None, edge_index=None) -> Tensor:
        """The attention read-out's node weights [N] of ONE graph (``readout="attention"`` only; same arguments as ``forward``,
        the tuple form included): the softmax of the gate's scores over the graph's nodes, on the device of ``x``.  No gradient."""
        if self.readout != "attention":
            raise ValueError(f"CombinedModel.attention_weights: readout is {self.readout!r}, not 'attention'")
        if pos is None and edge_index is None and isinstance(x, tuple):
            x, pos, edge_index = x
        dev = require_gpu_param(self.classifier.fc1.weight, "CombinedModel")
        back = x.device
        with torch.no_grad():
            x = x.to(device=dev, dtype=torch.float32)
            pos = pos.to(device=dev, dtype=torch.float32)
            # (pooled GraphNet: the survivors; padded layers: the rows in front of N', one read-back)
            y, ptr, _ = self.graph_net.forward_device(x, pos, get_topology(edge_index, x.size(0), dev), return_pooling=True,
                                                      compose_kept=False)
            if self.graph_net.pool_padded:
                y = y[:int(ptr[-1].item())]
            whole = torch.arange(2, dtype=torch.int64, device=dev) * y.size(0)  # [0, N], built on the device
            _, alpha = Fn.graph_attention_pool(y, self.gate.forward_segments([(y, None)]).view(-1), whole, return_weights=True)
        return alpha if back == dev else alpha.to(back)

    def kept_nodes(self, x, pos=None, edge_index=None) -> Tensor:
        """The nodes of ONE graph that survive the GraphNet's top-K pooling layers (``GraphNet(pool_ratio=...)`` only; same
        arguments as ``forward``, the tuple form included): int64 [N'] ORIGINAL node ids, ascending, on the device of ``x`` - on a
        superpixel graph, the map of the regions the read-out sees.  No gradient."""
        if not self.graph_net.pooling:
            raise ValueError("CombinedModel.kept_nodes: the GraphNet has no pooling layers (pool_ratio is None)")
        if pos is None and edge_index is None and isinstance(x, tuple):
            x, pos, edge_index = x
        dev = require_gpu_param(self.classifier.fc1.weight, "CombinedModel")
        back = x.device
        with torch.no_grad():
            x = x.to(device=dev, dtype=torch.float32)
            pos = pos.to(device=dev, dtype=torch.float32)
            _, ptr, kept = self.graph_net.forward_device(x, pos, get_topology(edge_index, x.size(0), dev), return_pooling=True)
            if self.graph_net.pool_padded:  # the N' survivors in front of the -1 tail: one read-back
                kept = kept[:int(ptr[-1].item())]
        kept = kept.long()
        return kept if back == dev else kept.to(back)

    def forward(self, x, pos=None, edge_index=None):
        """models/GNN.py:334-341; accepts the (x, pos, edge_index) tuple; logits are 1-D [classes]."""
        if pos is None and edge_index is None and isinstance(x, tuple):
            x, pos, edge_index = x
        dev = require_gpu_param(self.classifier.fc1.weight, "CombinedModel")
        back = x.device
        x = x.to(device=dev, dtype=torch.float32)
        pos = pos.to(device=dev, dtype=torch.float32)
        topo = get_topology(edge_index, x.size(0), dev)
        if self.graph_net.pool_padded:  # padded top-K pooling: all rows come back, graph_ptr' = [0, N'] says which are the graph's
            y, ptr, _ = self.graph_net.forward_device(x, pos, topo, return_pooling=True, compose_kept=False)
            if self.pooled:  # no read-back: the read-out takes rows through the device offsets
                logits = self.readout_logits(y, ptr)[0]
                return logits if back == dev else logits.to(back)
            y = y[:int(ptr[-1].item())]  # the flatten read-out is sized on the host: one read of N'
        else:
            y = self.graph_net.forward_device(x, pos, topo)  # (a pooled GraphNet: the survivors' rows, one graph)
        if self.pooled:
            logits = self.readout_logits(y, torch.arange(2, dtype=torch.int64, device=dev) * y.size(0))[0]  # [0, N], built on the device
            return logits if back == dev else logits.to(back)
        if self.ragged_readout and y.size(0) != self.num_nodes:
            y = ragged_readout_rows(y, self.num_nodes)  # full num_nodes * out_dim length: dW1 keeps fc1.weight's layout
        logits = self.classifier(y.flatten())
        return logits if back == dev else logits.to(back)

    def forward_batched(self, x, pos, edge_index, num_graphs: int | None = None, graph_ptr: Tensor | None = None):
        """Block-diagonal batch: one GraphNet pass over all graphs, then the read-out of all G graphs in the batched
        HIP read-out (``functional.readout_batched``; a shape it does not serve: one [G, num_nodes*out_dim] GEMM).  The reference has no batching (main.py:60);
        this equals G independent ``forward`` calls.

        * ``num_graphs`` given: every graph has exactly ``num_nodes`` nodes (graph g owns rows g*num_nodes ...).
        * ``graph_ptr`` [G+1] given (node offsets): graphs of ANY size.  The reference's read-out is only
          defined for N == num_nodes (its superpixel path crashes otherwise); the
          build-side rule, a stated deviation, is: the first ``num_nodes`` nodes of a graph feed ``fc1``, a
          smaller graph is zero-padded.  With N == num_nodes for every graph both modes coincide.
        """
        dev = require_gpu_param(self.classifier.fc1.weight, "CombinedModel")
        back = x.device
        x = x.to(device=dev, dtype=torch.float32)
        pos = pos.to(device=dev, dtype=torch.float32)
        topo = get_topology(edge_index, x.size(0), dev)
        if graph_ptr is None:
            if self.graph_net.pooling and not self.pooled:
                raise ValueError("forward_batched(num_graphs=...): behind top-K pooling (pool_ratio) the flatten read-out needs the "
                                 "graphs' offsets; pass graph_ptr")
            if num_graphs is None or x.size(0) != num_graphs * self.num_nodes:
                raise ValueError(f"expected num_graphs x {self.num_nodes} node rows (got {x.size(0)}); pass graph_ptr "
                                 f"for graphs of other sizes")
        else:
            graph_ptr = graph_ptr.to(device=dev, dtype=torch.int64)
        logits = self.forward_batched_device(x, pos, topo, num_graphs=num_graphs, graph_ptr=graph_ptr)
        return logits if back == dev else logits.to(back)

    def forward_batched_device(self, x, pos, topo: GraphTopology, num_graphs: int | None = None, graph_ptr: Tensor | None = None):
        """``forward_batched`` behind its topology lookup: float32 ``x`` / ``pos`` on the model's device, a prepared topology and
        either ``num_graphs`` (graph g owns rows ``[g * num_nodes, (g + 1) * num_nodes)``) or a DEVICE int64 ``graph_ptr``
        [G + 1].  ``x`` may hold more rows than the graphs own (the padded buffers of a captured ragged-batch step: slack and
        dummy rows behind ``graph_ptr[-1]``): the read-out takes rows through ``graph_ptr`` only.  No host synchronisation."""
        if self.pooled and graph_ptr is None:  # the num_graphs form: graph g owns rows [g * num_nodes, (g + 1) * num_nodes)
            graph_ptr = torch.arange(num_graphs + 1, dtype=torch.int64, device=x.device) * self.num_nodes
        if self.graph_net.pooling:  # K20: the read-out takes the POOLED graphs' offsets
            if graph_ptr is None:
                raise ValueError("forward_batched_device: behind top-K pooling (pool_ratio) the flatten read-out needs graph_ptr")
            y, graph_ptr, _ = self.graph_net.forward_device(x, pos, topo, graph_ptr=graph_ptr, return_pooling=True,
                                                            compose_kept=not self.graph_net.pool_padded)
            return self.readout_logits(y, graph_ptr)
        y = self.graph_net.forward_device(x, pos, topo)  # [N_total, out_dim]
        return self.readout_logits(y, graph_ptr, num_graphs)
