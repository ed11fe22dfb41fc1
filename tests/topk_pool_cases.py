"""Reference and cases of the top-K node pooling (K20).  No GPU here.

The reference is integer / float64 code that shares nothing with the kernels: the selection sorts each graph's rows with numpy's
``lexsort`` on (NaN last, larger score first, lower row first) - no keys, no radix, no scan; the edge filter is a boolean mask and a
cumulative sum; the gate and its backward are float64 torch.  ``pooled_forward`` composes the pooled GraphNet from the oracle's own
pieces (``O.mlp_forward``, ``O.edge_features``, ``O.gn_block``, ``O.classifier_forward``) with the selection above in between."""
import math

import numpy as np
import torch

from oracle import graphnet_oracle as O

SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16384)
RATIOS = (1.0, 0.8, 0.5, 0.25, 1e-3)
WIDTHS = (1, 3, 8, 64, 65, 128, 256)
CEIL_PAIRS = ((0.1, 10), (0.7, 10), (0.3, 10), (0.6, 5))  # ratio * n is an integer in exact arithmetic, not always in double
EDGE_TILE = 1024  # csrc/topk_pool_index.h: kEdgeTile
EDGE_COUNTS = (0, 1, 255, 256, 257, EDGE_TILE - 1, EDGE_TILE, EDGE_TILE + 1, 70001)


def keep_count(ratio: float, n: int) -> int:
    return min(n, max(1, math.ceil(ratio * n))) if n >= 1 else 0


def graph_ranges(graph_ptr, rows: int):
    """Clamped [a, b) per graph, as ``gnc_pool::graph_range``."""
    out = []
    for g in range(len(graph_ptr) - 1):
        a = min(max(int(graph_ptr[g]), 0), rows)
        b = min(max(int(graph_ptr[g + 1]), a), rows)
        out.append((a, b))
    return out


def ref_select(scores, graph_ptr, ratio: float):
    """``(new_id int32 [rows], kept int32 [N'], graph_ptr' int64 [G + 1])`` from scores of any float dtype (numpy)."""
    s = np.asarray(scores)
    rows = s.shape[0]
    nan = np.isnan(s)
    value = np.where(nan, 0.0, s) + 0.0  # (-0.0 + 0.0 = +0.0: the two zeros compare equal anyway)
    keep = np.zeros(rows, dtype=bool)
    gp = [0]
    for a, b in graph_ranges(graph_ptr, rows):
        k = keep_count(ratio, b - a)
        if k:
            idx = np.arange(a, b)
            order = np.lexsort((idx, -value[a:b], nan[a:b]))  # last key first: NaN last, then larger score, then lower row
            keep[idx[order[:k]]] = True
        gp.append(gp[-1] + k)
    kept = np.nonzero(keep)[0].astype(np.int32)
    new_id = np.full(rows, -1, dtype=np.int32)
    new_id[kept] = np.arange(kept.size, dtype=np.int32)
    return new_id, kept, np.asarray(gp, dtype=np.int64)


def ref_filter(src, dst, rowptr, new_id):
    """``(src', dst', kept_edges, edge_new_id, rowptr')`` of a destination-sorted edge list (int32 numpy)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    rows = new_id.shape[0]
    inside = (src >= 0) & (src < rows) & (dst >= 0) & (dst < rows)
    s = np.where(inside, new_id[np.clip(src, 0, max(rows - 1, 0))] if rows else -1, -1)
    d = np.where(inside, new_id[np.clip(dst, 0, max(rows - 1, 0))] if rows else -1, -1)
    keep = (s >= 0) & (d >= 0)
    kept_edges = np.nonzero(keep)[0].astype(np.int32)
    edge_new_id = np.full(src.shape[0], -1, dtype=np.int32)
    edge_new_id[kept_edges] = np.arange(kept_edges.size, dtype=np.int32)
    in_front = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)  # kept edges in front of position p, p = 0 ... E
    kept_nodes = np.nonzero(new_id >= 0)[0]
    rowptr_out = np.concatenate([in_front[np.asarray(rowptr, dtype=np.int64)[kept_nodes]], [kept_edges.size]]).astype(np.int32)
    return s[keep].astype(np.int32), d[keep].astype(np.int32), kept_edges, edge_new_id, rowptr_out


def ref_rows(x, scores, kept, grad=None):
    """float64: ``x' = x[kept] tanh(s[kept])`` (``scores`` None: no gate) and, with ``grad`` [N', C], ``(dx, ds)``."""
    x64 = torch.as_tensor(x).double().requires_grad_(True)
    s64 = torch.as_tensor(scores).double().requires_grad_(True) if scores is not None else None
    idx = torch.as_tensor(np.asarray(kept, dtype=np.int64))
    out = x64[idx] * torch.tanh(s64[idx])[:, None] if s64 is not None else x64[idx]
    if grad is None:
        return out.detach()
    out.backward(torch.as_tensor(grad).double())
    return out.detach(), x64.grad, (s64.grad if s64 is not None else None)


# ------------------------------------------------------------------------------------------------------------------ cases
def sorted_edges(rng, rows: int, E: int, hub: bool = False, self_loops: bool = True, out_of_range: int = 0):
    """A destination-sorted edge list over ``rows`` nodes: (src, dst, rowptr) int32.  ``hub``: one destination with 70 in-edges;
    ``out_of_range``: that many endpoints outside [0, rows) (negative and too large), kept in sorted position by their neighbours'
    destination (the filter must drop them without indexing)."""
    if rows == 0 or E == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(rows + 1, np.int32)
    dst = rng.integers(0, rows, size=E)
    if hub and E >= 70:
        dst[:70] = rows // 2
    src = rng.integers(0, rows, size=E)
    if self_loops:
        src[::7] = dst[::7]
    order = np.argsort(dst, kind="stable")
    src, dst = src[order].astype(np.int32), dst[order].astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=rows))]).astype(np.int32)
    for i in range(out_of_range):  # the CSR offsets still describe the list: a bad SOURCE keeps its slot
        p = int(rng.integers(0, E))
        src[p] = -1 - i if i % 2 else rows + i
    if out_of_range:  # bad DESTINATIONS sort in front of node 0 and behind the last node: rowptr[0] > 0 and rowptr[rows] < E
        front = np.array([-3, -1], np.int32)
        back = np.array([rows, rows + 5], np.int32)
        src = np.concatenate([np.array([0, rows - 1], np.int32), src, np.array([0, rows - 1], np.int32)])
        dst = np.concatenate([front, dst, back])
        rowptr = rowptr + np.int32(2)
    return src, dst, rowptr


def score_patterns(rng, n: int):
    """{name: float32 [n]}: the orders a selection can get wrong."""
    base = rng.standard_normal(n).astype(np.float32)
    out = {"random": base, "all_equal": np.full(n, 0.25, np.float32)}
    dup = np.round(base * 2).astype(np.float32) / 2  # a handful of distinct values: duplicates across every k boundary
    dup[dup == 0] = np.where(np.arange(n) % 2, 0.0, -0.0)[dup == 0]  # both zeros among the ties
    out["duplicates"] = dup
    special = base.copy()
    if n:
        special[rng.integers(0, n, size=max(1, n // 9))] = np.inf
        special[rng.integers(0, n, size=max(1, n // 9))] = -np.inf
        special[rng.integers(0, n, size=max(1, n // 7))] = np.nan
        special[rng.integers(0, n, size=max(1, n // 11))] = np.float32(-np.nan)
    out["special"] = special
    return out


# ------------------------------------------------------------------------------------------------------------------ model
def pooled_forward(sd, x, pos, ei, ratio, pool_after, graph_ptr=None, prefix="graph_net.", record=None):
    """The pooled GraphNet composed from the oracle's pieces in the dtype of ``sd``: ``(y [N', out_dim], graph_ptr', kept)`` with
    ``kept`` the survivors' original rows.  ``record``: a list that receives per pooling layer ``(scores, graph_ptr, kept mask)``."""
    n_blocks = O.n_blocks_of(sd, prefix)
    gp = np.asarray([0, x.size(0)] if graph_ptr is None else graph_ptr, dtype=np.int64)
    e = O.edge_features(pos, ei)
    h = O.mlp_forward(sd, prefix + "node_encoder", x)
    e = O.mlp_forward(sd, prefix + "edge_encoder", e)
    kept_all = np.arange(x.size(0))
    for b in range(n_blocks):
        if ei.size(1):
            h, e = O.gn_block(sd, f"{prefix}graph_processor.blocks.{b}", h, ei, e)
        else:  # a pooled graph without edges: no edge model to run, the node model sees an all-zero aggregate
            h = O.node_processor(sd, f"{prefix}graph_processor.blocks.{b}.node_model", h, ei, e)
        if b in pool_after:
            s = O.mlp_forward(sd, f"{prefix}graph_processor.pools.{b}.gate", h)[:, 0]
            new_id, kept, gp_out = ref_select(s.detach().numpy(), gp, ratio)
            if record is not None:
                record.append((s.detach(), gp.copy(), new_id >= 0))
            kidx = torch.from_numpy(kept.astype(np.int64))
            h = h[kidx] * torch.tanh(s[kidx])[:, None]
            nid = torch.from_numpy(new_id.astype(np.int64))
            alive = (nid[ei[0]] >= 0) & (nid[ei[1]] >= 0)
            ei, e = nid[ei[:, alive]], e[alive]
            kept_all, gp = kept_all[kept], gp_out
    return O.mlp_forward(sd, prefix + "node_decoder", h), gp, kept_all


def pooled_logits(sd, x, pos, ei, ratio, pool_after, readout, graph_ptr=None, record=None):
    """Logits [G, classes] of ``CombinedModel(GraphNet(pool_ratio=ratio), readout=readout)`` (``"mean"`` / ``"attention"``)."""
    y, gp, kept = pooled_forward(sd, x, pos, ei, ratio, pool_after, graph_ptr, record=record)
    rows = []
    for g in range(len(gp) - 1):
        yg = y[int(gp[g]):int(gp[g + 1])]
        if readout == "attention":
            alpha = torch.softmax(O.mlp_forward(sd, "gate", yg)[:, 0], dim=0)
            rows.append(O.classifier_forward(sd, alpha @ yg))
        else:
            rows.append(O.classifier_forward(sd, yg.mean(0)))
    return torch.stack(rows), kept
