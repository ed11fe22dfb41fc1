"""Reference of the capacity-padded top-K pooling layout.  No GPU here.

``ref_padded`` builds the padded arrays from ``topk_pool_cases.ref_select`` / ``ref_filter`` with plain Python integers (exact at any
size, no shared code with csrc/topk_pool_index.h): with N' / E' the kept counts, S_R = rows - N' and S_E = E - E',

* ``kept[N':] = -1`` and ``kept_edges[E':] = -1``;
* the edge at E' + t is a self-loop of slack row ``N' + t * S_R // S_E``;
* ``rowptr'[N' + u] = E' + ceil(u * S_E / S_R)`` for ``0 <= u <= S_R``, so ``rowptr'[rows] = E``;
* S_R == 0 with S_E > 0 (only edges with an endpoint outside ``[0, rows)`` can have been dropped): the slack edges loop on row
  ``rows - 1`` and ``rowptr'[rows] = E``.
"""
import numpy as np

from tests import topk_pool_cases as K


def ceil_div(a: int, b: int) -> int:
    return -((-a) // b)


def ref_padded(scores, graph_ptr, ratio: float, src=None, dst=None, rowptr=None):
    """``dict`` of the padded layer's integer outputs (numpy): ``new_id`` [rows], ``kept`` [rows], ``graph_ptr`` [G + 1], ``n_out`` and,
    with an edge list, ``src`` / ``dst`` / ``kept_edges`` / ``edge_new_id`` [E], ``rowptr`` [rows + 1], ``e_out``."""
    new_id, kept, gp = K.ref_select(scores, graph_ptr, ratio)
    rows, n_out = int(new_id.shape[0]), int(kept.size)
    out = {"new_id": new_id, "graph_ptr": gp, "n_out": n_out,
           "kept": np.concatenate([kept, np.full(rows - n_out, -1, np.int32)]).astype(np.int32)}
    if src is None:
        return out
    s, d, kept_edges, edge_new_id, rp = K.ref_filter(src, dst, rowptr, new_id)
    E, e_out = int(np.asarray(src).shape[0]), int(kept_edges.size)
    s_r, s_e = rows - n_out, E - e_out
    if s_r > 0:
        loops = [n_out + t * s_r // s_e for t in range(s_e)]
        tail = [e_out + ceil_div(u * s_e, s_r) for u in range(1, s_r + 1)]
        rp = np.concatenate([rp, np.asarray(tail, dtype=np.int64)]).astype(np.int32)
    else:
        loops = [rows - 1] * s_e
        rp = rp.copy()
        rp[rows] = E
    loops = np.asarray(loops, dtype=np.int32)
    out.update({"src": np.concatenate([s, loops]).astype(np.int32), "dst": np.concatenate([d, loops]).astype(np.int32),
                "kept_edges": np.concatenate([kept_edges, np.full(s_e, -1, np.int32)]).astype(np.int32),
                "edge_new_id": edge_new_id, "rowptr": rp, "e_out": e_out})
    return out
