"""Case builders, the float64 CPU reference and the error bars of the attention neighbourhood aggregation (K21), shared by
tests/test_segment_softmax_host.py, tests/test_gpu_segment_softmax.py and tests/test_gpu_attention_aggregation_model.py.  No GPU.

The reference is plain torch on the CPU in float64, one destination at a time (``segment_reduce_cases._segments``: the rows of
``src`` with ``index == v`` in ascending row order):
  m[v] = the largest score that is not a NaN (-inf for none; 0 for no rows), Z[v] = sum exp(s_k - m[v]),
  alpha_k = exp(s_k - m[v]) / Z[v], out[v] = sum alpha_k x_k; 0 and (m, Z) = (0, 0) for no rows;
  backward = the chain rule of exactly that.

Error bars, from each case's own float64 quantities: u = 2^-24, dmax_v = max_k |s_k - m_v|, c_v = 2 deg_v + 2 dmax_v + 12 -
recursive summation in numerator and Z (2 deg), the rounding of s - m carried through expf (a relative 2 dmax u at most, as
|s - m| <= dmax), expf's own error counted twice because e_k enters both sums, and the division (the constant):
  forward     |out - ref| <= c_v u sum_k alpha_k |x_k|
  grad_src    |err| <= c_v u |alpha_k grad_out[d, c]|
  grad_score  |err| <= (c_v + D) u alpha_k sum_c |grad_out[d, c]| (|x_k[c]| + sum_j alpha_j |x_j[c]|)
"""
import torch

from tests import segment_reduce_cases as R

U = 2.0 ** -24
SCALES = (1, 3, 8)
SMALL_N, SMALL_E, SMALL_WIDTHS, CHUNK_WIDTHS = R.SMALL_N, R.SMALL_E, R.SMALL_WIDTHS, R.CHUNK_WIDTHS
small_index, chunk_index, values, degrees = R.small_index, R.chunk_index, R.values, R.degrees
# the backward's xor tree over a row's lanes also reads the idle lanes of a group: 12 is 4 lanes with one idle, 100 is 32 with seven
BACKWARD_WIDTHS = SMALL_WIDTHS + (12, 100)


def scores_for(rows: int, scale: float, seed: int) -> torch.Tensor:
    """float32 [rows]: randn * scale."""
    return torch.randn(rows, generator=torch.Generator().manual_seed(1000 + seed), dtype=torch.float32) * float(scale)


def small_case(width: int, scale: float):
    """(index [211], src [211, width], scores [211], grad_out [37, width]) of the small regime, seeded by width and scale."""
    return (small_index(), values(SMALL_E, width, seed=width), scores_for(SMALL_E, scale, seed=width + scale),
            values(SMALL_N, width, seed=30 + width))


# ---------------------------------------------------------------------------------------------------------------- reference
def ref_attention(src: torch.Tensor, scores: torch.Tensor, index: torch.Tensor, num_nodes: int):
    """(out [N, D], alpha [E], m [N], Z [N]), all float64."""
    x, s = src.double(), scores.double().reshape(-1)
    out = torch.zeros(num_nodes, x.size(1), dtype=torch.float64)
    alpha = torch.zeros(s.numel(), dtype=torch.float64)
    m = torch.zeros(num_nodes, dtype=torch.float64)
    z = torch.zeros(num_nodes, dtype=torch.float64)
    for v, rows in enumerate(R._segments(index, num_nodes)):
        if not rows.numel():
            continue
        sv = s[rows]
        finite = sv[~torch.isnan(sv)]
        m[v] = finite.max() if finite.numel() else float("-inf")
        e = torch.exp(sv - m[v])
        z[v] = e.sum()
        alpha[rows] = e / z[v]
        out[v] = (e[:, None] * x[rows]).sum(0) / z[v]  # equal scores: e = 1 and this is the mean, exactly
    return out, alpha, m, z


def ref_weighted_abs(src: torch.Tensor, scores: torch.Tensor, index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """float64 [N, D]: sum_k alpha_k |x_k|, the scale of the forward bar."""
    return ref_attention(src.abs(), scores, index, num_nodes)[0]


def ref_attention_backward(grad_out: torch.Tensor, src: torch.Tensor, scores: torch.Tensor, index: torch.Tensor, num_nodes: int):
    """(grad_src [E, D], grad_scores [E]) in float64."""
    out, alpha, _, _ = ref_attention(src, scores, index, num_nodes)
    g = grad_out.double()[index.long()]
    return alpha[:, None] * g, alpha * (g * (src.double() - out[index.long()])).sum(1)


def error_constants(scores: torch.Tensor, index: torch.Tensor, num_nodes: int):
    """(deg [N], dmax [N], c [N]) in float64: c_v = 2 deg_v + 2 dmax_v + 12."""
    s = scores.double().reshape(-1)
    deg = R.degrees(index, num_nodes).double()
    dmax = torch.zeros(num_nodes, dtype=torch.float64)
    for v, rows in enumerate(R._segments(index, num_nodes)):
        if rows.numel():
            dmax[v] = (s[rows] - s[rows].max()).abs().max()
    return deg, dmax, 2 * deg + 2 * dmax + 12


def bars(src, scores, index, num_nodes, grad_out=None):
    """{"forward": [N, D], "saved_z": [N], "alpha": [E], and with ``grad_out`` "grad_src": [E, D], "grad_score": [E]}; "ref" holds
    the ``ref_attention`` tuple they were computed from."""
    idx = index.long()
    ref = ref_attention(src, scores, index, num_nodes)
    out, alpha, _, z = ref
    deg, dmax, c = error_constants(scores, index, num_nodes)
    wabs = ref_weighted_abs(src, scores, index, num_nodes)
    b = {"forward": c[:, None] * U * wabs, "saved_z": (deg + 2 * dmax + 8) * U * z, "alpha": c[idx] * U * alpha, "ref": ref}
    if grad_out is not None:
        g = grad_out.double()[idx]
        b["grad_src"] = c[idx][:, None] * U * (alpha[:, None] * g).abs()
        b["grad_score"] = (c[idx] + src.size(1)) * U * alpha * (g.abs() * (src.double().abs() + wabs[idx])).sum(1)
    return b


# --------------------------------------------------------------------------------- the same formulas in fp32 torch on the CPU
def fp32_attention(src: torch.Tensor, scores: torch.Tensor, index: torch.Tensor, num_nodes: int):
    """(out, alpha) in float32 with torch's vectorised ops: what an fp32 evaluation of the formulas gives (seed conditions)."""
    idx, s = index.long(), scores.float().reshape(-1)
    m = torch.full((num_nodes,), float("-inf")).scatter_reduce(0, idx, s, "amax")
    e = torch.exp(s - m[idx])
    z = torch.zeros(num_nodes).index_add_(0, idx, e)
    num = torch.zeros(num_nodes, src.size(1)).index_add_(0, idx, e[:, None] * src.float())
    out = torch.where(z[:, None] > 0, num / z.clamp(min=1e-30)[:, None], torch.zeros(()))
    return out, e / z[idx]


def fp32_attention_backward(grad_out, src, scores, index, num_nodes):
    out, alpha = fp32_attention(src, scores, index, num_nodes)
    g = grad_out.float()[index.long()]
    return alpha[:, None] * g, alpha * (g * (src.float() - out[index.long()])).sum(1)


def fraction(err: torch.Tensor, bar: torch.Tensor) -> float:
    """Largest err / bar (0 where both are 0; inf where an error stands against a zero bar)."""
    err, bar = err.double().flatten(), bar.double().flatten()
    ratio = torch.where(bar > 0, err / bar.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------- stand-in for the oracle's _scatter
class OracleAttentionScatter:
    """``oracle.graphnet_oracle._scatter(edge_attr, col, dim_size)`` replaced through monkeypatch by an instance: block b's call
    (the calls of one forward arrive in block order) scores the edge latents with that block's gate weights from ``sd`` and returns
    the softmax-weighted sums.  Differentiable, in the dtype of its input: the float64 autograd reference and the fp32 oracle."""

    def __init__(self, sd: dict, prefix: str = "graph_net."):
        from oracle import graphnet_oracle as O
        self.sd, self.prefix, self.blocks, self.calls, self._mlp = sd, prefix, O.n_blocks_of(sd, prefix), 0, O.mlp_forward
        self.alphas = []

    def __call__(self, src: torch.Tensor, index: torch.Tensor, dim_size: int) -> torch.Tensor:
        b = self.calls % self.blocks
        self.calls += 1
        idx = index.long()
        s = self._mlp(self.sd, f"{self.prefix}graph_processor.blocks.{b}.node_model.gate", src).reshape(-1)
        m = torch.full((dim_size,), float("-inf"), dtype=s.dtype).scatter_reduce(0, idx, s.detach(), "amax")
        e = torch.exp(s - m[idx])
        z = s.new_zeros(dim_size).index_add(0, idx, e)
        alpha = e / z[idx]
        self.alphas.append(alpha.detach())
        return src.new_zeros((dim_size, src.size(1))).index_add(0, idx, alpha[:, None] * src)


def hand_example():
    """5 destinations, 8 rows, 2 columns: destination 3 is empty, destination 4 has one row, destination 1 has three rows with
    EQUAL scores (its answer is the mean), destination 0 two rows whose scores differ by ln 3 (weights 1/4 and 3/4), destination 2
    two rows of which one is scored -inf (weight 0).  Returns (src, scores, index, out, alpha) with the answers written by hand."""
    import math
    index = torch.tensor([0, 1, 0, 2, 1, 4, 1, 2])
    src = torch.tensor([[1.0, -1.0],    # -> 0, score 0
                        [2.0, -0.5],    # -> 1
                        [3.0, 5.0],     # -> 0, score ln 3
                        [-4.0, 0.5],    # -> 2
                        [2.0, 0.0],     # -> 1
                        [7.0, -7.0],    # -> 4
                        [-6.0, -3.5],   # -> 1
                        [9.0, 9.0]])    # -> 2, score -inf
    scores = torch.tensor([0.0, 3.25, math.log(3.0), 1.5, 3.25, -2.0, 3.25, float("-inf")], dtype=torch.float64)
    out = torch.tensor([[2.5, 3.5], [-2.0 / 3.0, -4.0 / 3.0], [-4.0, 0.5], [0.0, 0.0], [7.0, -7.0]], dtype=torch.float64)
    alpha = torch.tensor([0.25, 1 / 3, 0.75, 1.0, 1 / 3, 1.0, 1 / 3, 0.0], dtype=torch.float64)
    return src, scores, index, out, alpha
