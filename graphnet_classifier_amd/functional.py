"""Autograd-aware operators over the HIP kernels.

Forward passes run in ``libgnc_hip.so`` (see :mod:`graphnet_classifier_amd.native`).  The
reference's only caller that needs gradients is ``utils/train_model.py:41``
(``loss.backward()``):

* scatter-sum backward is a row gather (HIP kernel K2);
* the fused-MLP backward runs on the hand-written K8 kernels (every width class up to 256); the training
  forward of the widths <= 64 kernels keeps the hidden layers' post-activations for it, the wider ones
  recompute the forward of each tile from the inputs (``GNC_TORCH_BACKWARD=1`` switches to a PyTorch-ROCm
  recompute for A/B runs; nothing here ever runs on the CPU);
* the three Functions around that kernel pair - ``_FusedMLP``, ``_WideFirstMLP``, ``_EdgeProcessorWSplit`` - share one record of a
  call (``_MlpCall``: the non-tensor facts and the flat order of the tensor arguments, their saved copies and their gradients),
  one assembly of the parameter gradients (``_parameter_grads``), one gradient of a gathered table and one PyTorch recompute
  chain;
* an MLP over ONE wide table (the image-MLP baseline: 49152 inputs, 8 rows) runs its first Linear on the split-K kernels K16 and
  the rest of its chain as an ordinary fused-MLP call, tied together by ``_WideFirstMLP`` (``GNC_NO_WIDE_LINEAR=1`` keeps the
  row-tiled kernels everywhere, for A/B runs);
* batch normalisation over table rows (``norm_type='BatchNorm1d'``) runs on the K14 kernels both ways.
"""
from __future__ import annotations

import collections

import torch
import torch.nn.functional as F

import os

from . import native

# GNC_TORCH_BACKWARD=1 keeps the PyTorch-ROCm recompute backward everywhere (A/B and parity checks)
HIP_BACKWARD = os.environ.get("GNC_TORCH_BACKWARD") is None


def _node_projections(x, w0, dn):
    """(x Ws^T, x Wd^T) [N, H] each: the per-node halves of the W-split first Linear (models/GNN.py:58-61).  ONE launch with two
    output tables for a small batch at 128 features and for a large batch at widths <= 64 (c3: rows read once, both column
    slices resident), two launches otherwise.  (One launch over the stacked weight [Ws ; Wd] writing ONE [N, 2H] table, the
    halves as gather tables, measured no faster - c3 8.14 / 8.29 vs 8.13 / 8.25 ms per step, c2 41.51 vs 41.55 - and was dropped.)"""
    return native.dual_projection(x, w0[:, :dn], w0[:, dn:2 * dn])


class _ScatterSumCSR(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, rowptr, perm, dst_of_row, num_nodes):
        ctx.save_for_backward(dst_of_row)
        return native.scatter_sum_csr(src, rowptr, perm, num_nodes)

    @staticmethod
    def backward(ctx, grad_out):
        (dst_of_row,) = ctx.saved_tensors  # d out[dst(e)] / d src[e] = I
        return native.gather_rows(grad_out.contiguous(), dst_of_row), None, None, None, None


def scatter_sum_csr(src: torch.Tensor, rowptr: torch.Tensor, perm, dst_of_row: torch.Tensor, num_nodes: int):
    """out[v] = sum of src rows whose destination is v.  ``perm`` maps sorted position ->
    row of ``src`` (None when ``src`` is already destination-sorted); ``dst_of_row[r]`` is the
    destination of ``src`` row r (int32), used by the backward gather."""
    return _ScatterSumCSR.apply(src, rowptr, perm, dst_of_row, num_nodes)


class _SegmentMeanCSR(torch.autograd.Function):
    """K18 mean (csrc/segment_reduce.hip): keeps nothing but the topology."""

    @staticmethod
    def forward(ctx, src, rowptr, perm, dst_of_row, num_nodes):
        ctx.save_for_backward(dst_of_row, rowptr)
        return native.segment_reduce_csr(src, rowptr, perm, num_nodes, native.SEGMENT_MEAN)[0]

    @staticmethod
    def backward(ctx, grad_out):
        dst_of_row, rowptr = ctx.saved_tensors  # d out[dst(e)] / d src[e] = I / deg(dst(e))
        return native.segment_reduce_backward(grad_out, dst_of_row, rowptr, None, native.SEGMENT_MEAN), None, None, None, None


class _SegmentMaxCSR(torch.autograd.Function):
    """K18 max: the winners' rows are stored only when a gradient will need them or the caller asks for them."""

    @staticmethod
    def forward(ctx, src, rowptr, perm, dst_of_row, num_nodes, want_argmax):
        need = ctx.needs_input_grad[0]
        out, argmax = native.segment_reduce_csr(src, rowptr, perm, num_nodes, native.SEGMENT_MAX, with_argmax=need or want_argmax)
        if need:
            ctx.save_for_backward(dst_of_row, rowptr, argmax)
        if argmax is None:
            return out, None
        ctx.mark_non_differentiable(argmax)
        return out, argmax

    @staticmethod
    def backward(ctx, grad_out, _grad_argmax=None):
        dst_of_row, rowptr, argmax = ctx.saved_tensors  # the gradient of a column goes to the row that won it, and only there
        return native.segment_reduce_backward(grad_out, dst_of_row, rowptr, argmax, native.SEGMENT_MAX), None, None, None, None, None


def segment_mean_csr(src: torch.Tensor, rowptr: torch.Tensor, perm, dst_of_row: torch.Tensor, num_nodes: int):
    """out[v] = mean of the src rows whose destination is v (+0.0 for none): the ascending sum of ``scatter_sum_csr`` divided by
    ``float(deg)``.  Arguments as ``scatter_sum_csr``; ``dst_of_row`` may be None when no gradient is wanted."""
    if dst_of_row is None and src.requires_grad and torch.is_grad_enabled():
        raise ValueError("segment_mean_csr: dst_of_row is needed for the backward")
    return _SegmentMeanCSR.apply(src, rowptr, perm, dst_of_row, num_nodes)


def segment_max_csr(src: torch.Tensor, rowptr: torch.Tensor, perm, dst_of_row: torch.Tensor, num_nodes: int,
                    return_argmax: bool = False):
    """out[v] = column-wise maximum of the src rows whose destination is v (+0.0 for none; a NaN wins; a tie goes to the lowest
    sorted position).  ``return_argmax``: ``(out, argmax)`` with ``argmax`` int32 [num_nodes, D], the winning row of ``src``, -1
    for a destination without rows.  Without it, and without autograd, the launch stores no winners."""
    if dst_of_row is None and src.requires_grad and torch.is_grad_enabled():
        raise ValueError("segment_max_csr: dst_of_row is needed for the backward")
    out, argmax = _SegmentMaxCSR.apply(src, rowptr, perm, dst_of_row, num_nodes, bool(return_argmax))
    return (out, argmax) if return_argmax else out


class _SegmentSoftmaxCSR(torch.autograd.Function):
    """K21 (csrc/segment_softmax.hip): keeps src, scores, out and the per-destination (max, sum of exp); no [E] weights."""

    @staticmethod
    def forward(ctx, src, scores, rowptr, perm, dst_of_row, num_nodes):
        out, saved = native.segment_softmax_csr(src, scores, rowptr, perm, num_nodes)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(src, scores, out, saved, dst_of_row)
        ctx.scores_shape = scores.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        src, scores, out, saved, dst_of_row = ctx.saved_tensors
        grad_src, grad_scores = native.segment_softmax_backward(grad_out, src, scores, out, saved, dst_of_row)
        return grad_src, grad_scores.view(ctx.scores_shape), None, None, None, None


def segment_softmax_csr(src: torch.Tensor, scores: torch.Tensor, rowptr: torch.Tensor, perm, dst_of_row: torch.Tensor, num_nodes: int):
    """out[v] = sum_k alpha_k src[k] over the rows whose destination is v, ``alpha`` the softmax of their ``scores`` (+0.0 for no
    rows; equal scores give the bits of ``segment_mean_csr``).  ``scores``: one float per row of ``src`` ([E] or [E, 1]), indexed as
    ``src`` is.  Other arguments as ``scatter_sum_csr``; ``dst_of_row`` may be None when no gradient is wanted."""
    if dst_of_row is None and (src.requires_grad or scores.requires_grad) and torch.is_grad_enabled():
        raise ValueError("segment_softmax_csr: dst_of_row is needed for the backward")
    return _SegmentSoftmaxCSR.apply(src, scores, rowptr, perm, dst_of_row, num_nodes)


class _DivByDegree(torch.autograd.Function):
    """Rows of an [N, D] aggregate divided by the in-degree (gnc_rows_div_degree_f32); linear, so the same launch on the gradient."""

    @staticmethod
    def forward(ctx, agg, rowptr, inplace):
        ctx.save_for_backward(rowptr)
        if inplace:
            ctx.mark_dirty(agg)
            return native.rows_div_degree_(agg, rowptr)
        return native.rows_div_degree_(agg.clone(memory_format=torch.contiguous_format), rowptr)

    @staticmethod
    def backward(ctx, grad_out):
        (rowptr,) = ctx.saved_tensors
        return native.rows_div_degree_(grad_out.clone(memory_format=torch.contiguous_format), rowptr), None, None


def div_by_degree(agg: torch.Tensor, rowptr: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """``agg[v] / float(deg(v))`` for the per-destination sums ``agg`` [N, D] of a CSR (rows of degree 0 unchanged): with
    ``scatter_sum_csr`` - or the edge launch's aggregation epilogue - in front of it, the bits of ``segment_mean_csr``.
    ``inplace=True`` overwrites ``agg`` (the caller owns it and nothing else reads the sums)."""
    return _DivByDegree.apply(agg, rowptr, bool(inplace))


class _PermuteRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, perm, inv_perm):
        ctx.save_for_backward(inv_perm)
        return native.gather_rows(table, perm)

    @staticmethod
    def backward(ctx, grad_out):
        (inv_perm,) = ctx.saved_tensors
        return native.gather_rows(grad_out.contiguous(), inv_perm), None, None


def permute_rows(table: torch.Tensor, perm: torch.Tensor, inv_perm: torch.Tensor) -> torch.Tensor:
    """out[k] = table[perm[k]] for a permutation ``perm`` (int32) with inverse ``inv_perm``."""
    return _PermuteRows.apply(table, perm, inv_perm)


def _torch_activation(name: str, param: float):
    if name == "LeakyReLU":
        return lambda v: F.leaky_relu(v, param)
    if name == "ELU":
        return lambda v: F.elu(v, param)
    return {"ReLU": F.relu, "Identity": lambda v: v, "Tanh": torch.tanh, "Sigmoid": torch.sigmoid, "SiLU": F.silu,
            "GELU": F.gelu}[name]


_MlpArgs = collections.namedtuple("_MlpArgs", "tables weights biases ln residual")


class _MlpCall:
    """One fused-MLP call: its non-tensor facts, and the flat layout of its tensor arguments - tables, weights, biases,
    (gamma, beta behind a LayerNorm), (residual if any).  That order is the one of the arguments behind the record in
    ``Function.apply``, of ``needs_input_grad`` and the saved tensors, and of the gradients a backward returns; nothing else
    knows it.  There are as many tables as ``indices``: one (or None) per segment - for the W-split edge processor the tables
    (x, e) and the two gathers (src, dst) of x."""
    __slots__ = ("indices", "num_tables", "num_linear", "activation", "act_param", "ln_eps", "has_ln", "has_residual", "rows",
                 "with_agg", "training")

    def __init__(self, indices, num_linear, activation, act_param, ln, residual, rows, with_agg=False):
        self.indices, self.num_tables = tuple(indices), len(indices)
        self.num_linear, self.activation, self.act_param = num_linear, activation, float(act_param)
        self.has_ln, self.ln_eps = ln is not None, float(ln[2]) if ln is not None else 0.0
        self.has_residual, self.rows, self.with_agg = residual is not None, int(rows), bool(with_agg)
        # the caller's grad mode (inside Function.forward it is always off): a backward can only follow when it was on
        self.training = torch.is_grad_enabled()

    def pack(self, tables, weights, biases, ln=None, residual=None) -> tuple:
        """The flat tuple of the named groups; of ``ln`` its first two entries (gamma, beta) go in."""
        return (*tables, *weights, *biases, *(ln[:2] if self.has_ln else ()), *((residual,) if self.has_residual else ()))

    def unpack(self, flat) -> _MlpArgs:
        """The named groups of a flat tuple - arguments, ``needs_input_grad`` flags or gradients; ``ln`` is (gamma, beta, eps) as
        the kernels take it, or None."""
        s = self.num_tables
        w = s + self.num_linear
        b = w + self.num_linear
        ln = (flat[b], flat[b + 1], self.ln_eps) if self.has_ln else None
        return _MlpArgs(list(flat[:s]), list(flat[s:w]), list(flat[w:b]), ln, flat[-1] if self.has_residual else None)

    def tables(self, flat):
        """The tables' entries of a flat tuple alone (what a forward asks of ``needs_input_grad``)."""
        return flat[:self.num_tables]

    def split_saved(self, saved):
        """(the flat arguments, whatever the forward saved behind them) of a node's ``saved_tensors``."""
        n = self.num_tables + 2 * self.num_linear + 2 * self.has_ln + self.has_residual
        return saved[:n], list(saved[n:])

    def grads(self, need, tables=None, weights=None, biases=None, gamma=None, beta=None, residual=None) -> tuple:
        """The gradient tuple a backward returns behind the non-tensor arguments: gradients given by name, table k / weight l /
        bias l as the k-th / l-th entry of their lists; None for a group left out and wherever ``need`` says no."""
        flat = self.pack(tables or [None] * self.num_tables, weights or [None] * self.num_linear,
                         biases or [None] * self.num_linear, (gamma, beta), residual)
        return tuple([g if n else None for g, n in zip(flat, need)])


def _torch_recompute_backward(call: _MlpCall, flat, need, grad_out, first_input, residual=lambda a: a.residual):
    """GNC_TORCH_BACKWARD=1 (A/B and parity runs only): PyTorch-ROCm recompute backward of the same ops on the GPU.
    ``first_input(tables)`` is the first Linear's input, ``residual(args)`` what is added behind the norm (or None)."""
    leaves = [a.detach().requires_grad_(bool(n)) for a, n in zip(flat, need)]
    a = call.unpack(leaves)
    act = _torch_activation(call.activation, call.act_param)
    with torch.enable_grad():
        h = first_input(a.tables)
        for k, (w, b) in enumerate(zip(a.weights, a.biases)):
            h = F.linear(h, w, b)
            if k + 1 < call.num_linear:
                h = act(h)
        if a.ln is not None:
            h = F.layer_norm(h, (h.size(-1),), *a.ln)
        if residual(a) is not None:
            h = h + residual(a)
        wanted = [x for x, n in zip(leaves, need) if n]
        grads = iter(torch.autograd.grad(h, wanted, grad_out.contiguous(), allow_unused=True))
    return tuple(next(grads) if n else None for n in need)


def _gathered_table_grad(row_grads, table, idx):
    """Gradient of ``table`` from the gradients of the rows a segment read from it.  Rows gathered by index (operator-level
    API only): summed per table row with K1 through the index's own destination CSR - stable order, no float atomics,
    bitwise reproducible."""
    if idx is None:
        return row_grads
    from .topology import get_destination_csr
    csr = get_destination_csr(idx, table.size(0), table.device)
    return native.scatter_sum_csr(row_grads, csr.rowptr, csr.perm, table.size(0))


def _parameter_grads(r, blocks, need_w, need_b, need_ln, grad_out):
    """``([dW_l], [db_l], dgamma, dbeta)`` of one MLP backward from ``r``, the result of ``native.mlp_backward``; None where the
    flags ``need_w[l]`` / ``need_b[l]`` / ``need_ln`` ((gamma, beta), or None without a LayerNorm) do not ask.  dW_l = dz_l^T (input
    of Linear l), db_l = column sums of dz_l.  ``blocks``: the column blocks of dW_0 in concat order as (left, right) operands,
    dW_0[:, block] = left^T right; a block whose left operand is dz_0 itself is the data kernel's own first Linear: the first of
    them gives db_0, and the fused kernel hands them - like every later layer - out itself (``r["dw"]`` / ``r["db"]``).  Every
    other product of the layers asked for, and the row sums of the LayerNorm partials, are ONE xty_multi call (one launch for
    a small batch), the blocks of dW_0 written in place."""
    fused, dz0, num_linear = "dw" in r, r["dz"][0], len(need_w)
    dw, db = [None] * num_linear, [None] * num_linear
    products, slots = [], []  # slots[i]: the layer that takes (dW, db) of product i - of dW_0's blocks only db - or None
    if need_w[0] or need_b[0]:
        own = [left is dz0 for left, _ in blocks]
        if fused:
            db[0] = r["db"][0]
        if fused and all(own):
            dw[0] = r["dw"][0]
        else:
            dw[0] = torch.empty(blocks[0][0].size(1), sum(right.size(1) for _, right in blocks), dtype=torch.float32,
                                device=blocks[0][1].device)
            off = 0
            for (left, right), mine in zip(blocks, own):
                out = dw[0][:, off:off + right.size(1)]
                off += right.size(1)
                if fused and mine:
                    out.copy_(r["dw"][0])
                else:
                    products.append((left, right, out))
                    slots.append(0 if mine and 0 not in slots else None)
    for k in range(1, num_linear):
        if not (need_w[k] or need_b[k]):
            continue
        if fused:
            dw[k], db[k] = r["dw"][k], r["db"][k]
        else:
            products.append((r["dz"][k], r["act"][k - 1], None))
            slots.append(k)
    ln_part = r.get("ln_part")
    res, sums = native.xty_multi(products, [ln_part] if ln_part is not None else []) if (products or ln_part is not None) else ([], [])
    for k, (c, cs) in zip(slots, res):
        if k is not None:
            dw[k], db[k] = (c if k > 0 else dw[0]), cs
    dgamma = dbeta = None
    if need_ln is not None:
        if ln_part is not None:
            od = ln_part.size(1) // 2
            dbeta, dgamma = sums[0][:od], sums[0][od:]
        else:
            dbeta, dgamma = r["ln_sums"] if r["ln_sums"] is not None else native.colsum_pair(grad_out, r["yhat"])
        dgamma, dbeta = dgamma if need_ln[0] else None, dbeta if need_ln[1] else None
    return [g if n else None for g, n in zip(dw, need_w)], [g if n else None for g, n in zip(db, need_b)], dgamma, dbeta


class _FusedMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, call: _MlpCall, *flat):
        a = call.unpack(flat)
        # training forward: the kernel also leaves the hidden layers' post-activations (what autograd would keep) for K8
        acts = [] if (call.training and any(ctx.needs_input_grad) and HIP_BACKWARD) else None
        out = native.mlp_forward(list(zip(a.tables, call.indices)), a.weights, a.biases, ln=a.ln,
                                 activation=call.activation, act_param=call.act_param, residual=a.residual, rows=call.rows,
                                 save_act=acts, save_need_dx=any(call.tables(ctx.needs_input_grad[1:])))
        ctx.call = call
        # the saved post-activations go through save_for_backward like the inputs: autograd then frees them as soon as this
        # node's backward has run (held as plain attributes they lived until the whole graph died: +30 GB at c5)
        ctx.save_for_backward(*flat, *(acts or []))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        call, need = ctx.call, ctx.needs_input_grad[1:]
        flat, acts = call.split_saved(ctx.saved_tensors)
        if call.rows == 0:  # no rows: every gradient is a zero of its argument's shape (an edge-less graph, superpixel.py:70-71)
            return (None,) + tuple(torch.zeros_like(a) if n else None for a, n in zip(flat, need))
        if HIP_BACKWARD:
            hip = _fused_mlp_backward_hip(call, flat, need, grad_out, acts or None)
            if hip is None:  # an activation other than ReLU (or a shape outside K8): layer by layer, still on this library
                hip = _layerwise_mlp_backward_hip(call, flat, need, grad_out)
            return (None,) + hip
        return (None,) + _torch_recompute_backward(call, flat, need, grad_out, lambda tables: torch.cat(
            [t if i is None else t[i.long()] for t, i in zip(tables, call.indices)], dim=-1))


def _fused_mlp_backward_hip(call: _MlpCall, flat, need, grad_out, saved_act=None):
    """Backward of one fused-MLP call on the HIP kernels (K8): data path + one skinny GEMM per Linear.
    Returns the gradient tuple in argument order, or None when the shape is outside the kernels."""
    a, n = call.unpack(flat), call.unpack(need)
    segments = list(zip(a.tables, call.indices))
    if (call.activation != "ReLU" or call.num_linear < 2 or not grad_out.is_cuda
            or not native.mlp_backward_supported(segments, a.weights, a.biases, a.ln, call.activation, a.residual, call.rows,
                                                 saved_act=saved_act)):
        return None
    grad_out = grad_out.contiguous()
    r = native.mlp_backward(segments, a.weights, a.biases, a.ln, grad_out, rows=call.rows, need_dx=any(n.tables),
                            saved_act=saved_act, defer_ln_sums=True)
    # inputs: dx is in concat (= weight column) order, and so are the column blocks of dW_0 = dz_0^T [rows of every segment]
    off, dtables, blocks = 0, [], []
    for (t, idx), wanted in zip(segments, n.tables):
        w = t.size(1)
        blocks.append((r["dz"][0], t if idx is None else native.gather_rows(t, idx)))
        dtables.append(_gathered_table_grad(r["dx"][:, off:off + w], t, idx) if wanted else None)
        off += w
    dw, db, dgamma, dbeta = _parameter_grads(r, blocks, n.weights, n.biases, n.ln, grad_out)
    return call.grads(need, dtables, dw, db, dgamma, dbeta, grad_out)


def _layerwise_mlp_backward_hip(call: _MlpCall, flat, need, grad_out):
    """Backward of one fused-MLP call for the shapes the K8 kernels do not take - an activation other than ReLU
    (models/MLP.py:21 accepts any nn.<Name>) - layer by layer on the library's own kernels: the pre-activations are
    recomputed with single-Linear K4 launches, act / act' / the LayerNorm backward are row-wise kernels
    (csrc/elementwise.hip), da = dz W is a single-Linear launch on the transposed weight, dW = dz^T a and db come from
    gnc_xty_f32, gathered segments get their gradient through K1.  Nothing here is on the path of a ReLU model."""
    p, n = call.unpack(flat), call.unpack(need)
    l, weights, biases = call.num_linear, p.weights, p.biases
    act, ap = call.activation, call.act_param
    if act not in native.ACTIVATIONS or not grad_out.is_cuda:
        raise NotImplementedError(f"backward of an MLP with activation nn.{act} has no HIP kernel")
    segments = list(zip(p.tables, call.indices))
    grad_out = grad_out.contiguous()
    # forward recompute: z_k (pre-activations) and a_k = act(z_k)
    zs, acts = [], []
    z = native.mlp_forward(segments, [weights[0]], [biases[0]], activation="Identity", rows=call.rows)
    for k in range(l):
        zs.append(z)
        if k + 1 < l:
            a = native.activation(z, act, ap)
            acts.append(a)
            z = native.mlp_forward([(a, None)], [weights[k + 1]], [biases[k + 1]], activation="Identity")
    dtables, dw, db = [], [None] * l, [None] * l
    dz, dgamma, dbeta = grad_out, None, None
    if p.ln is not None:
        dz, yhat = native.layer_norm_backward(zs[-1], p.ln[0], grad_out, call.ln_eps)
        if n.ln[0] or n.ln[1]:
            dbeta, dgamma = native.colsum_pair(grad_out, yhat)
    for k in range(l - 1, 0, -1):
        if n.weights[k] or n.biases[k]:
            dw[k], db[k] = native.xty(dz, acts[k - 1])
        da = native.mlp_forward([(dz, None)], [weights[k].t().contiguous()], [None], activation="Identity")  # dz W_k
        dz = native.activation_backward(zs[k - 1], da, act, ap)
    # first Linear: its input is the virtual concat of the segments (gathered ones materialised for the products)
    off, parts = 0, []
    for (t, idx), wanted in zip(segments, n.tables):
        w = t.size(1)
        if n.weights[0] or n.biases[0]:
            c, cs = native.xty(dz, t if idx is None else native.gather_rows(t, idx))
            parts.append(c)
            db[0] = cs if db[0] is None else db[0]
        dtables.append(_gathered_table_grad(native.mlp_forward([(dz, None)], [weights[0][:, off:off + w].t().contiguous()], [None],
                                                               activation="Identity"), t, idx) if wanted else None)
        off += w
    if n.weights[0]:
        dw[0] = torch.cat(parts, dim=1) if len(parts) > 1 else parts[0]
    return call.grads(need, dtables, dw, db, dgamma, dbeta, grad_out)


class _WideFirstMLP(torch.autograd.Function):
    """A fused-MLP call over ONE wide row-ordered table: the first Linear + activation on K16 (csrc/wide_linear.hip), the remaining
    Linears + LayerNorm as an ordinary fused-MLP launch over its output; the backward of that launch supplies the gradient of the
    first Linear's output (its ``need_dx``), from which K16 forms dW0 and db0.  The table itself gets no gradient (it is data: the
    route is not taken when it wants one)."""

    @staticmethod
    def forward(ctx, call: _MlpCall, *flat):
        a = call.unpack(flat)
        training = call.training and any(ctx.needs_input_grad)
        relu = call.activation == "ReLU"
        a0, z0 = native.wide_linear_forward(a.tables[0], a.weights[0], a.biases[0], call.activation, call.act_param,
                                            want_z=training and not relu)
        acts = [] if training else None
        out = native.mlp_forward([(a0, None)], a.weights[1:], a.biases[1:], ln=a.ln, activation=call.activation,
                                 act_param=call.act_param, rows=call.rows, save_act=acts, save_need_dx=True)
        ctx.call = call
        if training:
            ctx.save_for_backward(*flat, a0, a0 if relu else z0, *(acts or []))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        call, need = ctx.call, ctx.needs_input_grad[1:]
        flat, (a0, az, *acts) = call.split_saved(ctx.saved_tensors)
        a, n = call.unpack(flat), call.unpack(need)
        # the rest of the chain, as the fused-MLP call over a0 that the forward made
        rest = _MlpCall((None,), call.num_linear - 1, call.activation, call.act_param, a.ln, None, call.rows)
        rest_flat, rest_need = rest.pack([a0], a.weights[1:], a.biases[1:], a.ln), rest.pack([True], n.weights[1:], n.biases[1:], n.ln)
        g = _fused_mlp_backward_hip(rest, rest_flat, rest_need, grad_out, acts or None)
        if g is None:  # an activation other than ReLU, or a single Linear behind the first: layer by layer, still on this library
            g = _layerwise_mlp_backward_hip(rest, rest_flat, rest_need, grad_out)
        g = rest.unpack(g)
        dw0 = db0 = None
        if n.weights[0] or n.biases[0]:
            dw0, db0 = native.wide_linear_backward(g.tables[0], az, a.tables[0], call.activation, call.act_param)
        dgamma, dbeta = g.ln[:2] if g.ln is not None else (None, None)
        return (None,) + call.grads(need, None, [dw0] + g.weights, [db0] + g.biases, dgamma, dbeta)


def wide_linear_route(segments, weights, biases, ln, activation, residual, rows) -> bool:
    """Does this fused-MLP call run its first Linear on K16?  One plain table that wants no gradient, and the library's own
    decision (native.wide_linear_serves) about everything else.  ``GNC_NO_WIDE_LINEAR=1`` (read on every call) says no."""
    if len(segments) != 1 or residual is not None or os.environ.get("GNC_NO_WIDE_LINEAR") is not None or not HIP_BACKWARD:
        return False
    if segments[0][0].requires_grad and torch.is_grad_enabled():
        return False  # K16 does not form the gradient of its input
    return native.wide_linear_serves(segments, weights, biases, ln, activation, residual, rows)


def fused_mlp(segments, weights, biases, ln=None, activation: str = "ReLU", act_param: float = 0.0, residual=None,
              rows: int | None = None) -> torch.Tensor:
    """segments: list of (table fp32 [*, w], index int32 [rows] | None); see native.mlp_forward."""
    tables = [t for t, _ in segments]
    indices = tuple(i for _, i in segments)
    if rows is None:
        rows = indices[0].numel() if indices[0] is not None else tables[0].size(0)
    call = _MlpCall(indices, len(weights), activation, act_param, ln, residual, rows)
    fn = _WideFirstMLP if wide_linear_route(segments, weights, biases, ln, activation, residual, rows) else _FusedMLP
    return fn.apply(call, *call.pack(tables, weights, biases, ln, residual))


class _BatchNormRows(torch.autograd.Function):
    """Training-mode batch norm over table rows (K14, csrc/batchnorm.hip), residual add fused into the apply launch."""

    @staticmethod
    def forward(ctx, z, gamma, beta, residual, running_mean, running_var, momentum, eps):
        out, mean, invstd = native.bn_forward(z, gamma, beta, residual, running_mean, running_var, momentum, eps)
        ctx.save_for_backward(z, mean, invstd, gamma)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        z, mean, invstd, gamma = ctx.saved_tensors
        need = ctx.needs_input_grad
        dz = dgamma = dbeta = None
        if need[0] or need[1] or need[2]:
            dz, dgamma, dbeta = native.bn_backward(grad_out, z, mean, invstd, gamma, need_dz=need[0])
        # x_hat is recomputed from z in both launches; the residual's gradient is grad_out itself (no copy)
        return (dz, dgamma if need[1] else None, dbeta if need[2] else None, grad_out if need[3] else None, None, None, None, None)


def batch_norm_rows(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, residual: torch.Tensor | None,
                    running_mean: torch.Tensor | None, running_var: torch.Tensor | None, momentum: float, eps: float,
                    training: bool = True, inplace: bool = False) -> torch.Tensor:
    """``nn.BatchNorm1d`` in training mode on ``z`` [rows, C] (C <= 256) plus an optional residual, on the K14 kernels: batch
    statistics (biased variance) normalise the rows, the running statistics - when given - are updated in place with
    ``momentum``.  ``inplace``: the caller does not need ``z`` afterwards; honoured when no gradient is wanted (the backward
    reads ``z``).  Eval mode has no operator of its own: an eval-mode module folds the normalisation into its last Linear
    (``native.bn_fold``)."""
    if not training:
        raise NotImplementedError("batch_norm_rows: eval mode is served by folding the normalisation into the last Linear "
                                  "(native.bn_fold), not by this operator")
    if z.dim() != 2:
        raise ValueError(f"batch_norm_rows: expected a [rows, C] table, got shape {tuple(z.shape)}")
    if z.size(0) == 1:  # torch.nn.functional.batch_norm's check, before any launch
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {z.size()}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (z, gamma, beta, residual)):
        return _BatchNormRows.apply(z, gamma, beta, residual, running_mean, running_var, float(momentum), float(eps))
    return native.bn_forward(z, gamma, beta, residual, running_mean, running_var, float(momentum), float(eps), inplace=inplace)[0]


class _EdgeProcessorWSplit(torch.autograd.Function):
    """EdgeProcessor (models/GNN.py:57-64) on destination-sorted edges with the first Linear
    split algebraically:  W0 [x_src | x_dst | e]^T = Ws x[src] + Wd x[dst] + We e.
    Two per-NODE projection launches (num_linear == 1, no bias) + one per-EDGE launch whose
    first two segments are gathered and ADDED.  The record's tables are (x, e), its indices (src, dst)."""

    @staticmethod
    def forward(ctx, call: _MlpCall, topo, *flat):
        a = call.unpack(flat)
        (x, e), (src, dst), w0 = a.tables, call.indices, a.weights[0]
        dn = x.size(1)
        ps, pd = _node_projections(x, w0, dn)                                 # [N, H] = x Ws^T, x Wd^T
        training = call.training and any(ctx.needs_input_grad) and HIP_BACKWARD
        acts = [] if training else None   # the hidden layers' post-activations, kept for K8 where the kernel can
        out = native.mlp_forward([(ps, src), (pd, dst), (e, None)], [w0[:, 2 * dn:]] + a.weights[1:], a.biases, ln=a.ln,
                                 activation=call.activation, act_param=call.act_param, residual=e, rows=call.rows,
                                 modes=[native.SEG_ADD, native.SEG_ADD, native.SEG_MATMUL],
                                 aggregate=(topo.dst_sorted, topo.rowptr, topo.num_nodes) if call.with_agg else None,
                                 save_act=acts, save_need_dx=bool(call.tables(ctx.needs_input_grad[2:])[1]))
        ctx.call, ctx.topo = call, topo
        ctx.set_materialize_grads(False)  # an unused output (the last block's e') arrives as None, not as zeros
        # kept for the backward through save_for_backward (freed when this node's backward has run): the projections - its
        # gathered inputs again, [N, H] each - and the post-activations
        ctx.save_for_backward(*flat, *(([ps, pd] + acts) if training else []))
        if not call.with_agg:
            return out
        out, agg = out
        if agg is None:  # the launch shape cannot carry the epilogue: K1 as a separate launch
            agg = native.scatter_sum_csr(out, topo.rowptr, None, topo.num_nodes)
        return out, agg

    @staticmethod
    def backward(ctx, grad_out, grad_agg=None):
        call, need = ctx.call, ctx.needs_input_grad[2:]
        if not call.with_agg:
            grad_agg = None
        if grad_out is None and grad_agg is None:
            return (None, None) + tuple(None for _ in need)
        flat, extra = call.split_saved(ctx.saved_tensors)
        if call.rows == 0:  # an edge-less graph (superpixel.py:70-71): zeros of every argument's shape
            return (None, None) + tuple(torch.zeros_like(a) if n else None for a, n in zip(flat, need))
        # e' feeds the aggregation (its backward is a row gather by destination: grad_agg[dst]) AND whatever consumed e'
        # itself (grad_out): the K8 launch adds the gathered rows itself where its kernel can
        if HIP_BACKWARD:
            hip = _edge_wsplit_backward_hip(call, ctx.topo, flat, extra, need, grad_out, grad_agg)
            if hip is None:  # (EdgeProcessor.forward_sorted only takes the W-split route for shapes K8 serves)
                raise NotImplementedError("W-split edge processor: this shape has no HIP backward kernel (use the concat form)")
            return (None, None) + hip
        src, dst = call.indices
        if grad_agg is not None and grad_out is not None:
            grad_out = native.gather_rows_add(grad_agg.contiguous(), dst, grad_out.contiguous())
        elif grad_agg is not None:
            grad_out = native.gather_rows(grad_agg.contiguous(), dst)
        return (None, None) + _torch_recompute_backward(
            call, flat, need, grad_out, lambda t: torch.cat([t[0][src.long()], t[0][dst.long()], t[1]], dim=-1),
            residual=lambda a: a.tables[1])


def _edge_wsplit_backward_hip(call: _MlpCall, topo, flat, extra, need, grad_out, grad_agg=None):
    """HIP backward of the W-split edge processor.  Per edge: the K8 data kernel (recompute + chain),
    then dz0 is (i) the gradient of both gathered projections - summed per node through the two CSRs
    (destination-sorted: the forward's; source-sorted: topo.csc) - and (ii) the left operand of dWe.
    ``extra``: what the training forward kept behind the arguments (ps, pd, post-activations), or nothing."""
    a, n = call.unpack(flat), call.unpack(need)
    (x, e), (src, dst), w0 = a.tables, call.indices, a.weights[0]
    if topo is None or call.activation != "ReLU" or not (grad_out if grad_out is not None else grad_agg).is_cuda:
        return None
    dn = x.size(1)
    # the forward's projections are needed again as the gathered additive inputs (kept by the training forward)
    ps, pd, *acts = extra or _node_projections(x, w0, dn)
    segments = [(ps, src), (pd, dst), (e, None)]
    modes = [native.SEG_ADD, native.SEG_ADD, native.SEG_MATMUL]
    wl = [w0[:, 2 * dn:]] + a.weights[1:]
    if not native.mlp_backward_supported(segments, wl, a.biases, a.ln, call.activation, e, call.rows, modes):
        return None
    r = native.mlp_backward(segments, wl, a.biases, a.ln, grad_out.contiguous() if grad_out is not None else None, rows=call.rows,
                            modes=modes, need_dx=bool(n.tables[1]), residual=e,
                            grad_gather=(grad_agg.contiguous(), dst) if grad_agg is not None else None,
                            saved_act=acts or None, defer_ln_sums=True)
    grad_out = r["grad_out"]  # effective row-ordered gradient (None when the launch gathered part of it itself)
    dz0 = r["dz"][0]
    de = None
    if n.tables[1]:  # through We, plus the residual path (folded into the kernel's dx when it can)
        de = r["dx"] if r["residual_folded"] else r["dx"] + grad_out
    # node side: d(ps)[v] = sum of dz0 over edges with src == v, d(pd)[v] = ... dst == v
    csc_rowptr, csc_perm = topo.csc
    dps = native.scatter_sum_csr(dz0, csc_rowptr, csc_perm, topo.num_nodes)
    dpd = native.scatter_sum_csr(dz0, topo.rowptr, None, topo.num_nodes)
    # dx = dps Ws + dpd Wd: one projection launch over [dps | dpd] with the weight [Ws ; Wd]^T
    # (a small batch reads W0 transposed, in one launch, without the copy)
    dx = native.projection_t2(dps, dpd, w0, dn) if n.tables[0] else None
    # dW_0 = [dps^T x | dpd^T x | dz0^T e]; the layers behind the first are formed whether or not their parameters train
    behind = [True] * (call.num_linear - 1)
    dw, db, dgamma, dbeta = _parameter_grads(r, [(dps, x), (dpd, x), (dz0, e)], n.weights[:1] + behind, n.biases[:1] + behind,
                                             n.ln, grad_out)
    return call.grads(need, (dx, de), dw, db, dgamma, dbeta)


def edge_processor_wsplit(x, e, topo, weights, biases, ln, activation="ReLU", act_param=0.0, with_agg=False):
    """``with_agg=True`` returns ``(e', agg)``: the per-destination sums come from the edge launch's epilogue (or
    from K1 when that launch cannot carry it) and both outputs are differentiable."""
    call = _MlpCall((topo.src_sorted, topo.dst_sorted), len(weights), activation, act_param, ln, None, e.size(0), with_agg=with_agg)
    return _EdgeProcessorWSplit.apply(call, topo, *call.pack((x, e), weights, biases, ln))


def edge_processor_wsplit_aggregated(x, e, topo, weights, biases, ln, activation="ReLU", act_param=0.0, store_edges=True):
    """Inference form of ``edge_processor_wsplit`` (no autograd graph): the edge launch also forms the
    per-destination sums of its output rows in its epilogue (include/gnc_hip.h, ``agg_out``).
    Returns ``(e', agg)``; ``agg`` is None when the launch shape cannot carry the epilogue (the caller then
    runs K1).  ``agg`` is bit-identical to ``scatter_sum_csr(e', topo.rowptr)``.  ``store_edges=False``: ``e'`` is not
    wanted, and where the aggregate-only launch serves the shape it is not stored either: ``(None, agg)``."""
    dn = x.size(1)
    w0 = weights[0]
    ps, pd = _node_projections(x, w0, dn)
    return native.mlp_forward([(ps, topo.src_sorted), (pd, topo.dst_sorted), (e, None)], [w0[:, 2 * dn:]] + list(weights[1:]),
                              list(biases), ln=ln, activation=activation, act_param=act_param, residual=e, rows=e.size(0),
                              modes=[native.SEG_ADD, native.SEG_ADD, native.SEG_MATMUL],
                              aggregate=(topo.dst_sorted, topo.rowptr, topo.num_nodes), agg_only=not store_edges)


class _Readout(torch.autograd.Function):
    """LinearClassifier.forward for ONE graph (models/GNN.py:312-325) as one launch each way (csrc/readout.hip)."""

    @staticmethod
    def forward(ctx, y, w1, b1, w2, b2, w3, b3):
        logits, h1, h2 = native.readout_forward(y, w1, b1, w2, b2, w3, b3)
        ctx.save_for_backward(y, w1, w2, w3, h1, h2)
        ctx.has_bias = (b1 is not None, b2 is not None, b3 is not None)
        return logits

    @staticmethod
    def backward(ctx, grad_logits):
        y, w1, w2, w3, h1, h2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy, dw1, db1, dw2, db2, dw3, db3 = native.readout_backward(grad_logits, y, w1, w2, w3, h1, h2, need_dy=need[0])
        hb = ctx.has_bias
        return (dy.view_as(y) if need[0] else None, dw1 if need[1] else None, db1 if (need[2] and hb[0]) else None,
                dw2 if need[3] else None, db2 if (need[4] and hb[1]) else None, dw3 if need[5] else None,
                db3 if (need[6] and hb[2]) else None)


def readout(y, w1, b1, w2, b2, w3, b3):
    """Single-graph read-out MLP; ``y`` 1-D float32 on the GPU."""
    return _Readout.apply(y, w1, b1, w2, b2, w3, b3)


class _ReadoutBatched(torch.autograd.Function):
    """LinearClassifier.forward over the G graphs of a block-diagonal batch with forward_batched's gather rule fused into fc1's
    operand load (csrc/readout_batched.hip): no [G, F] feature matrix, two launches forward."""

    @staticmethod
    def forward(ctx, y, graph_ptr, num_graphs, num_nodes, w1, b1, w2, b2, w3, b3):
        logits, h1, h2 = native.readout_batched_forward(y, graph_ptr, num_graphs, num_nodes, w1, b1, w2, b2, w3, b3)
        ctx.save_for_backward(y, graph_ptr, w1, w2, w3, h1, h2)
        ctx.shape = (num_graphs, num_nodes)
        ctx.has_bias = (b1 is not None, b2 is not None, b3 is not None)
        return logits

    @staticmethod
    def backward(ctx, grad_logits):
        y, graph_ptr, w1, w2, w3, h1, h2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy, dw1, db1, dw2, db2, dw3, db3 = native.readout_batched_backward(grad_logits, y, graph_ptr, ctx.shape[0], ctx.shape[1], w1, w2,
                                                                           w3, h1, h2, need_dy=need[0])
        hb = ctx.has_bias
        return (dy.view_as(y) if need[0] else None, None, None, None, dw1 if need[4] else None, db1 if (need[5] and hb[0]) else None,
                dw2 if need[6] else None, db2 if (need[7] and hb[1]) else None, dw3 if need[8] else None,
                db3 if (need[9] and hb[2]) else None)


def readout_batched(y, graph_ptr, num_graphs, num_nodes, w1, b1, w2, b2, w3, b3):
    """Read-out MLP of ``num_graphs`` graphs: ``y`` [N_total, out_dim] float32 on the GPU; ``graph_ptr`` int64 [G + 1] on the same
    device (graphs of any size: the first ``num_nodes`` rows of a graph feed fc1, a smaller graph is zero-padded) or None (graph g
    owns rows ``[g * num_nodes, (g + 1) * num_nodes)``).  Returns logits [G, C]."""
    return _ReadoutBatched.apply(y, graph_ptr, int(num_graphs), int(num_nodes), w1, b1, w2, b2, w3, b3)


class _ClassLoss(torch.autograd.Function):
    """Loss head (csrc/class_loss.hip, K23): the forward launch returns the loss AND d loss / d logits (with the loss accumulator,
    the confusion counts and the label check on the side); the backward is one multiply by the upstream gradient, on the device."""

    @staticmethod
    def forward(ctx, logits, labels, options, buffers):
        need = ctx.needs_input_grad[0]
        loss, dz = native.class_loss(logits, labels, with_gradient=need, **options, **buffers)
        if need:
            ctx.save_for_backward(dz)
        return loss.view(())

    @staticmethod
    def backward(ctx, grad_loss):
        (dz,) = ctx.saved_tensors
        return dz * grad_loss, None, None, None


def class_loss(logits: torch.Tensor, labels: torch.Tensor, *, kind: str = "ce", class_weight: torch.Tensor | None = None,
               label_smoothing: float = 0.0, pos_weight: float = 1.0, reduction: str = "mean", scale: float = 1.0,
               status: torch.Tensor | None = None, loss_sum: torch.Tensor | None = None, confusion: torch.Tensor | None = None,
               workspace: torch.Tensor | None = None) -> torch.Tensor:
    """0-dim loss of ``logits`` [G, C] float32 on the GPU and ``labels`` int64 [G] - or the reference's single-graph form, ``logits``
    [C] with a 0-dim label (models/GNN.py:338-341).  ``kind="ce"``: ``F.cross_entropy(logits, labels, weight=class_weight,
    label_smoothing=..., reduction=...)``; ``kind="bce"``: ``F.binary_cross_entropy_with_logits`` on ONE logit per sample with labels
    0 / 1 smoothed to ``y (1 - s) + s / 2`` and ``pos_weight``; both times ``scale``.  Differentiable in ``logits`` (scoring only when
    they need no gradient).  ``status`` (int32 [1]; made here when None) gets bit 0 when a label lies outside the classes - that sample
    is left out; ``loss_sum`` / ``confusion`` / ``workspace``: see ``native.class_loss``."""
    labels = torch.as_tensor(labels)
    if logits.dim() == 1 and labels.dim() == 0:
        logits, labels = logits.unsqueeze(0), labels.reshape(1)
    if logits.dim() != 2 or labels.dim() != 1:
        raise ValueError(f"class_loss: logits [G, C] with labels [G], or logits [C] with a 0-dim label, expected; got "
                         f"{tuple(logits.shape)} and {tuple(labels.shape)}")
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=logits.device)
    options = dict(kind=kind, class_weight=class_weight, label_smoothing=label_smoothing, pos_weight=pos_weight, reduction=reduction,
                   scale=scale)
    buffers = dict(status=status, loss_sum=loss_sum, confusion=confusion, workspace=workspace)
    return _ClassLoss.apply(logits, labels, options, buffers)


class _GraphPool(torch.autograd.Function):
    """Global pooling read-out over the graphs of a block-diagonal batch (csrc/pool_readout.hip, K17): one launch (two for a few
    large graphs) forward, one streaming launch backward."""

    @staticmethod
    def forward(ctx, y, graph_ptr, modes):
        out, argmax = native.graph_pool_forward(y, graph_ptr, modes)
        ctx.save_for_backward(graph_ptr, *([argmax] if argmax is not None else []))
        ctx.modes, ctx.rows = modes, y.size(0)
        return out

    @staticmethod
    def backward(ctx, grad):
        graph_ptr, *rest = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return native.graph_pool_backward(grad, ctx.modes, rest[0] if rest else None, graph_ptr, ctx.rows), None, None


def graph_pool(y: torch.Tensor, graph_ptr: torch.Tensor, mode: str) -> torch.Tensor:
    """Permutation-invariant read-out: ``y`` [rows, C] float32 on the GPU, ``graph_ptr`` int64 [G + 1] on the same device (graph g
    owns rows ``[graph_ptr[g], graph_ptr[g + 1])``; rows outside the graphs are ignored and receive zero gradient).  ``mode``
    ``"mean"`` / ``"max"`` / ``"sum"`` -> [G, C]; ``"hybrid"`` -> ``cat([mean, max, sum], dim=1)`` [G, 3C] from one pass.  An empty
    graph pools to zeros; the maximum's gradient goes to the lowest row that holds it."""
    if mode not in native.POOL_MODES:
        raise ValueError(f"graph_pool: mode {mode!r} is not one of {sorted(native.POOL_MODES)}")
    return _GraphPool.apply(y, graph_ptr, native.POOL_MODES[mode])


class _GraphAttentionPool(torch.autograd.Function):
    """Attention read-out over the graphs of a block-diagonal batch (csrc/attention_pool.hip, K19): one launch (three for a few
    large graphs) forward, one streaming launch backward that recomputes the weights from the per-graph (max, sum) it kept."""

    @staticmethod
    def forward(ctx, y, scores, graph_ptr):
        out, saved = native.graph_attention_pool_forward(y, scores, graph_ptr)
        ctx.save_for_backward(y, scores, graph_ptr, out, saved)
        ctx.mark_non_differentiable(saved)
        return out, saved

    @staticmethod
    def backward(ctx, grad, _grad_saved):
        y, scores, graph_ptr, out, saved = ctx.saved_tensors
        need_dy, need_ds = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dy, ds = native.graph_attention_pool_backward(grad, y, scores, out, saved, graph_ptr, need_dy, need_ds)
        return dy, ds, None


def graph_attention_pool(y: torch.Tensor, scores: torch.Tensor, graph_ptr: torch.Tensor, return_weights: bool = False):
    """Attention read-out: ``out[g] = sum_v alpha_v y[v]`` over the rows of graph g with ``alpha = softmax(scores[rows of g])``;
    ``y`` [rows, C] and ``scores`` [rows] float32 on the GPU, ``graph_ptr`` int64 [G + 1] on the same device (as ``graph_pool``'s:
    rows outside the graphs are ignored and receive zero gradient, an empty graph pools to zeros).  Differentiable in ``y`` and
    ``scores``.  ``return_weights=True``: ``(out, alpha)`` with ``alpha`` [rows] float32, zero outside the graphs, not
    differentiable."""
    out, saved = _GraphAttentionPool.apply(y, scores, graph_ptr)
    if not return_weights:
        return out
    return out, native.graph_attention_weights(scores.detach(), saved, graph_ptr)


class _TopKNodeRows(torch.autograd.Function):
    """Gated compaction of the node rows (csrc/topk_pool.hip, K20): ``x'[v'] = x[v] tanh(s_v)`` for the kept rows; one streaming
    launch each way, the backward writes every row of ``dx`` / ``ds`` once (exact +0.0 for a dropped row)."""

    @staticmethod
    def forward(ctx, x, scores, kept, new_id):
        out = native.topk_pool_rows_forward(x, kept, scores)
        ctx.save_for_backward(x, scores, new_id)
        return out

    @staticmethod
    def backward(ctx, grad):
        x, scores, new_id = ctx.saved_tensors
        dx, ds = native.topk_pool_rows_backward(grad, new_id, x, scores, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, ds, None, None


class _TopKEdgeRows(torch.autograd.Function):
    """Compaction of the edge rows without a gate (K20): ``e'[j'] = e[j]`` for the kept edges, ``de[j] = de'[j']`` or +0.0."""

    @staticmethod
    def forward(ctx, e, kept_edges, edge_new_id):
        ctx.save_for_backward(edge_new_id)
        return native.topk_pool_rows_forward(e, kept_edges)

    @staticmethod
    def backward(ctx, grad):
        (edge_new_id,) = ctx.saved_tensors
        return native.topk_pool_rows_backward(grad, edge_new_id)[0], None, None


def topk_pool(x: torch.Tensor, scores: torch.Tensor, topo, graph_ptr: torch.Tensor, ratio: float, edge_attr: torch.Tensor | None = None,
              need_edges: bool = True, padded: bool = False):
    """Top-K node pooling (K20): per graph of ``graph_ptr`` (device int64 [G + 1]) keep the ``k = min(n, max(1, ceil(ratio n)))``
    rows with the best ``scores`` [rows] - larger first, ``-0.0 == +0.0``, NaN last, ties by lower row - IN THEIR OLD ORDER, gate
    them (``x' = x tanh(s)``, so the scorer receives a gradient), and keep the edges of ``topo`` between two kept nodes, renumbered
    (still destination-sorted: no sort, no topology build).  ``edge_attr`` [E, De], in ``topo``'s sorted order, is compacted
    without a gate.  Returns ``(x', edge_attr' | None, topo', graph_ptr', kept)``; ``kept`` int32 [N'] are the survivors' old rows,
    ascending.  Differentiable in ``x``, ``scores`` and ``edge_attr``.

    ONE host synchronisation per call: the sizes N' and E' are read back from the device (a single read of both) to size the
    outputs, so this cannot run inside a hipGraph capture.  ``need_edges=False`` (nothing reads the pooled edges, e.g. behind the
    last GN block): nodes only, ``topo'`` is None and the read-back is of N' alone - still one.

    ``padded=True``: the capacity-padded form, NO host synchronisation, so a hipGraph capture can record it.  Every result keeps
    the input's size: ``x'`` [rows, C] and ``kept`` int32 [rows], ``edge_attr'`` [E, De], ``topo'`` over ``rows`` nodes and E edges.
    The first N' rows / E' edges are the sized form's; behind them ``x'`` and ``edge_attr'`` hold exact +0.0 rows, ``kept`` holds -1,
    and the slack edges are self-loops spread evenly over the slack rows ``[N', rows)``.  ``graph_ptr'`` ends at N', so the slack rows
    belong to no graph: a read-out ignores them, a later pooling layer erases them (and its edge filter their loops) again.  The
    blocks behind the layer run on all ``rows`` / E again - that is the price of the replay."""
    from .topology import GraphTopology
    scores = scores.reshape(-1)
    new_id, kept, gp_out, counts = native.topk_pool_select(scores.detach(), graph_ptr, ratio, padded=padded)
    if padded:  # counts stays on the device; the row launches run over the whole tables (a -1 id gives a +0.0 row)
        x_out = _TopKNodeRows.apply(x, scores, kept, new_id)
        if not need_edges:
            return x_out, None, None, gp_out, kept
        src, dst, kept_edges, edge_new_id, rowptr = native.topk_pool_filter_edges(topo.src_sorted, topo.dst_sorted, topo.rowptr, new_id,
                                                                                 kept, counts, padded=True)
        topo_out = GraphTopology.from_sorted(rowptr, src, dst, x.size(0), topo.status, topo.deferred)
        e_rows = _TopKEdgeRows.apply(edge_attr, kept_edges, edge_new_id) if edge_attr is not None else None
        return x_out, e_rows, topo_out, gp_out, kept
    if need_edges:
        src, dst, kept_edges, edge_new_id, rowptr = native.topk_pool_filter_edges(topo.src_sorted, topo.dst_sorted, topo.rowptr, new_id, kept,
                                                                                 counts)
        n_out, e_out = counts.tolist()  # the one read-back of this pooling layer
    else:
        n_out, e_out = int(counts[0].item()), 0
    kept = kept[:n_out]
    x_out = _TopKNodeRows.apply(x, scores, kept, new_id)
    if not need_edges:
        return x_out, None, None, gp_out, kept
    kept_edges = kept_edges[:e_out]
    topo_out = GraphTopology.from_sorted(rowptr[:n_out + 1], src[:e_out], dst[:e_out], n_out, topo.status, topo.deferred)
    e_rows = _TopKEdgeRows.apply(edge_attr, kept_edges, edge_new_id) if edge_attr is not None else None
    return x_out, e_rows, topo_out, gp_out, kept


def knn_graph(feat: torch.Tensor, k: int, graph_ptr=None, loop: bool = False, return_dist: bool = False, return_status: bool = False):
    """k-nearest-neighbour edges (K24): ``edge_index`` int64 [2, k N] in which slot ``v k + j`` holds the ``j``-th nearest row of
    ``v`` inside ``v``'s own graph as the sender and ``v`` as the receiver - receiver-major, in-degree exactly ``k``.  The distance is
    the squared Euclidean one over the columns of ``feat`` [N, D] (device float32, D <= 16, a strided row is read where it lies),
    summed in fp32 with ascending columns and no fused multiply-add; equal distances go to the smaller node id; ``loop`` admits the
    node itself.  The result is a pure function of the features' bits: the same alone, inside any batch and twice.

    ``graph_ptr``: int64 [G + 1] on the host (tensor, list) or the device; None is one graph.  On the host a graph with fewer than
    ``k`` candidates raises ``ValueError`` before anything is launched.  On the device nothing is read back: such a graph leaves -1
    in its unfillable slots and sets ``native.KNN_FEW_CANDIDATES`` in the status word, a NaN distance sets
    ``native.KNN_NAN_DISTANCE``; ``return_status=True`` appends that int32 [1] device tensor to the result.  One launch, no host
    synchronisation, capturable.  Not differentiable: indices come back, ``feat.requires_grad`` is ignored.

    Returns ``edge_index``, or a tuple ``(edge_index[, dist][, status])`` with ``dist`` float32 [k N] when asked."""
    if not isinstance(feat, torch.Tensor) or feat.dim() != 2:
        raise ValueError("knn_graph: feat must be a [N, D] tensor")
    feat = feat.detach()
    native._knn_feat(feat, k, "knn_graph")
    N = feat.size(0)
    if graph_ptr is None:
        graph_ptr = [0, N]
    if not isinstance(graph_ptr, torch.Tensor) or not graph_ptr.is_cuda:
        host = torch.as_tensor(graph_ptr, dtype=torch.int64).reshape(-1)
        if host.numel() < 2 or int(host[0]) != 0 or int(host[-1]) != N or bool((host[1:] < host[:-1]).any()):
            raise ValueError(f"knn_graph: graph_ptr must ascend from 0 to the {N} rows of feat")
        sizes = host[1:] - host[:-1]
        need = k if loop else k + 1
        small = torch.nonzero((sizes < need) & (sizes > 0)).reshape(-1)
        if small.numel():
            g = int(small[0])
            raise ValueError(f"knn_graph: graph {g} has {int(sizes[g])} nodes, fewer than the {need} that k = {k} needs"
                             f"{'' if loop else ' without self-loops'}")
        graph_ptr = host.to(feat.device)
    elif graph_ptr.dtype != torch.int64:
        raise ValueError(f"knn_graph: graph_ptr must be int64, got {graph_ptr.dtype}")
    edge_index, dist, status = native.knn_graph(feat, graph_ptr, k, loop=loop, return_dist=return_dist)
    out = (edge_index,) + ((dist,) if return_dist else ()) + ((status,) if return_status else ())
    return out[0] if len(out) == 1 else out


def edge_features(pos: torch.Tensor, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """[pos[dst]-pos[src], L1 norm] per edge (models/GNN.py:299-302).  ``pos`` is input data
    (utils/dataloader.py:50); gradients with respect to it are not provided."""
    if pos.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("gradients with respect to node positions are not implemented")
    return native.edge_features(pos, src, dst)
