"""Case table and float64 definitions of the fused-MLP family tests (tests/test_gpu_mlp_families.py on the GPU,
tests/test_mlp_family_cases_host.py for the check on the host that plain fp32 arithmetic meets the bars).

A case is a launch shape: segments in concat order (row-ordered or gathered, MATMUL or ADD), the widths of its Linear
layers, LayerNorm or none, the residual, optional ``None`` biases, operands that are column slices of wider tensors.
``build(name, rows)`` draws its host inputs (float32, CPU) from a seed and evaluates the float64 definition on them;
``build_backward(name, rows)`` adds ``grad_out`` and float64 autograd.  Row counts are not part of a case: the tests derive
them from the device (``derived_rows``).  Results are read-only and shared between the tests that need them.

The family ``generic`` holds the descriptions only the generic kernel (mlp_fused_kernel<HT, OT>, csrc/mlp_fused.hip) serves:
every multi-layer launch with an activation other than ReLU, and the ReLU descriptions all specialised kernels decline
(tests/test_gpu_mlp_generic.py).  ``activate`` applies the named activation through the same torch.nn.functional call in
float64 and float32.

ReLU kinks (LeakyReLU has the same one): a hidden pre-activation within ``KINK`` of zero in float64 may come out on the other
side in fp32 (the rounding of such a sum is about 1e-6), which moves a gradient by a whole weight column.  ``build_backward`` decides those rows from the
float64 forward alone and sets their ``grad_out`` rows to zero: a zero output-gradient row contributes exactly nothing to
dz, dx, the weight gradients and the LayerNorm sums whichever branch a kernel takes, so every output is compared in full."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch

SEG_MATMUL, SEG_ADD = 0, 1
TOL = 1e-5        # forward bar, times max(1, max|ref|)
DX_BAR = 2e-5     # dz[0] and dx, absolute      } the bars of test_mlp_backward_kernel_matches_autograd;
DW_BAR = 1e-4     # dW / db, times max(1, max|g|) } tests/test_mlp_family_cases_host.py shows that fp32 CPU autograd
LN_SUM_BAR = 1e-3  # d gamma / d beta, absolute  } meets the first two at 65,829 rows and all three at 16,421
# The LayerNorm sums grow with the row count (max|d gamma| is about 1000 at 65,829 rows): fp32 CPU autograd is 2.56e-3 off
# float64 there (bwd_edge_wsplit_128; 1.66e-3 at bwd_node_48, 1.52e-3 at bwd_plain_200), above 1e-3.  At rows_loop the bar is
# therefore 3 x that figure - the kernels sum in a different but equally long order.
LN_SUM_FP32_CPU_AT_LOOP = 2.56e-3
LN_SUM_BAR_LOOP = 3 * LN_SUM_FP32_CPU_AT_LOOP
KINK = 1e-5       # |z| below which a hidden pre-activation counts as a ReLU kink
KINK_SHARE = 0.01  # at most this share of the rows of a backward case may be marked
KINKED = ("ReLU", "LeakyReLU")  # activations whose derivative jumps at 0; the others are smooth and mark nothing
NODES = 2003      # rows of a gathered table
LN_EPS = 1e-5


def derived_rows(small_batch_rows: int, cu: int) -> dict:
    """first: the first row count the throughput forward sees (last tile: one row); loop: every family has more tiles than its
    persistent grid has waves, last tile ragged; bwd: the first size on the 8-wave streamed backward instances; small16 /
    two_wave: the last sizes on the 2-wave instances of the 16-row and of the 32-row streaming kernels, which serve a
    65..128-wide launch below the small-batch limit where the column-split kernel declines it."""
    return {"small": 777, "first": small_batch_rows + 1, "loop": max(small_batch_rows, 256 * cu) + 256 + 37,
            "bwd": 2 * 32 * cu + 32 + 5, "small16": 2 * 16 * cu - 3, "two_wave": 2 * 32 * cu - 5}


MI355X_ROWS = derived_rows(128 * 256, 256)  # first 32,769, loop 65,829, bwd 16,421 (small16 8,189, two_wave 16,379)


@dataclass(frozen=True)
class Case:
    name: str
    family: str            # stream (65..128) | resident (<= 64) | stream16 (129..256) | split1 | split2 | generic
    segs: tuple            # ((width, None | "src" | "dst", mode), ...) in concat order
    dims: tuple            # out width of every Linear
    ln: bool = True
    res: int | None = None  # the segment whose rows are the residual
    nobias: tuple = ()     # Linear layers without a bias
    sliced: bool = False   # tables and weights are column slices of wider tensors (ld > width)
    shared: bool = False   # the gathered segments read one table
    k6: bool = False       # the [rows, 3] table is the edge features of (pos, src, dst): the K6 prologue computes it
    activation: str = "ReLU"  # nn.<Name> between the Linear layers
    act_param: float = 0.0    # LeakyReLU's negative slope, ELU's alpha

    @property
    def in_dim(self) -> int:
        return sum(w for w, _, m in self.segs if m == SEG_MATMUL)

    @property
    def modes(self) -> list:
        return [m for _, _, m in self.segs]


def _plain(i, dims, **kw):
    return dict(segs=((i, None, SEG_MATMUL),), dims=tuple(dims), **kw)


def _shape(shape: str, d: int, layers: int = 3, ln: bool = True) -> dict:
    """The launch shapes of the model at width ``d`` (``layers`` Linear layers)."""
    dims = (d,) * layers
    if shape == "plain":
        return _plain(d, dims, ln=ln)
    if shape == "encoder3":   # nn.Linear(3, d) on [rows, 3]: nothing is a 16-B piece
        return _plain(3, dims, ln=ln)
    if shape == "projection":
        return _plain(d, (d,), ln=False, nobias=(0,))
    if shape == "edge_wsplit":  # two gathered ADD segments (the pre-multiplied projections) + e, residual e
        return dict(segs=((d, "src", SEG_ADD), (d, "dst", SEG_ADD), (d, None, SEG_MATMUL)), dims=dims, ln=ln, res=2)
    if shape == "node":        # [x | agg], residual x
        return dict(segs=((d, None, SEG_MATMUL), (d, None, SEG_MATMUL)), dims=dims, ln=ln, res=0)
    if shape == "decoder":
        return _plain(d, dims[:-1] + (1,), ln=False)
    if shape == "decoder5":
        return _plain(d, dims[:-1] + (5,), ln=False)
    if shape == "concat_edge":  # the concat form: two GATHERED matmul segments of one table + e; first Linear without bias
        return dict(segs=((d, "src", SEG_MATMUL), (d, "dst", SEG_MATMUL), (d, None, SEG_MATMUL)), dims=(d, d), ln=ln, res=2,
                    nobias=(0,), shared=True)
    raise KeyError(shape)


def _cases():
    out = []

    def add(name, family, **kw):
        out.append(Case(name=name, family=family, **kw))

    # ---- 32-row streaming kernel (hidden / out width 65..128) above the small-batch limit
    for d in (128, 100):
        for shape in ("encoder3", "projection", "edge_wsplit", "node", "decoder", "concat_edge"):
            add(f"stream_{shape}_{d}", "stream", **_shape(shape, d))
    add("stream_h100", "stream", **dict(_plain(100, (100, 100, 100)), res=0))  # no width a multiple of 16: masks everywhere
    add("stream_two_linears", "stream", **_plain(96, (128, 72), ln=False))
    add("stream_sliced_node_128", "stream", **dict(_shape("node", 128), sliced=True))
    add("stream_L4_128", "stream", **_shape("plain", 128, layers=4))
    # five Linear layers are more weight chunks than the column-split kernel holds: it declines, and the 2-wave instances of
    # mlp_stream16 (up to 2 * 16 * CUs rows) and of mlp_stream (up to 2 * 32 * CUs) serve the small batch
    add("stream_L5_100", "stream", **_shape("plain", 100, layers=5))
    # ---- weights-resident kernel (<= 64): one 32-column tile (16, 20, 32) and two (40, 48, 52)
    for d in (16, 20, 32, 40, 48, 52):
        for shape in ("plain", "node", "concat_edge", "decoder"):
            add(f"resident_{shape}_{d}", "resident", **_shape(shape, d))
    for d in (16, 20, 32):  # (at 33..64 this shape is split class 1, below)
        add(f"resident_edge_wsplit_{d}", "resident", **_shape("edge_wsplit", d))
    for d in (20, 52):
        add(f"resident_decoder5_{d}", "resident", **_shape("decoder5", d))
        add(f"resident_noln_{d}", "resident", **_shape("plain", d, ln=False))
        add(f"resident_L2_{d}", "resident", **_shape("plain", d, layers=2))
        add(f"resident_L4_{d}", "resident", **_shape("plain", d, layers=4))
    # a narrow output (<= 32) behind a shape that is not plain: the weights-resident kernel declines, mlp_stream<2, 1, 8> serves
    add("resident_narrow_node_48_5", "resident", segs=((48, None, SEG_MATMUL), (48, None, SEG_MATMUL)), dims=(48, 48, 5), ln=False)
    # ---- 16-row streaming kernel (129..256)
    for d in (136, 200):
        for shape in ("plain", "node", "edge_wsplit", "decoder"):
            add(f"stream16_{shape}_{d}", "stream16", **_shape(shape, d))
    add("stream16_160_256_72", "stream16", **_plain(160, (256, 72)))
    # ---- split class 1 off its c3 shape: the W-split edge processor at any width 33..64
    for d in (36, 40, 48, 52, 60):
        add(f"split1_L3_{d}", "split1", **_shape("edge_wsplit", d))
        add(f"split1_L2_noln_{d}", "split1", **_shape("edge_wsplit", d, layers=2, ln=False))
    # ---- split class 2: encoders behind a 64-wide hidden layer, first Linear K <= 4
    for od in (40, 52, 64):
        add(f"split2_table4_{od}", "split2", **_plain(4, (64, 64, od)))
        add(f"split2_rows3_{od}", "split2", **_plain(3, (64, 64, od)))
    add("split2_table4_L2_48", "split2", **_plain(4, (64, 48)))
    add("split2_rows3_L2_48", "split2", **_plain(3, (64, 48)))
    add("split2_k6_64", "split2", **_plain(3, (64, 64, 64), k6=True))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SPLIT_FAMILIES = ("split1", "split2")


def forward_rows(case: Case) -> tuple:
    """Keys of ``derived_rows`` a forward case runs at."""
    if case.k6:
        return ("loop",)  # the prologue serves batches above the small-batch limit only
    if case.name == "stream_L5_100":
        return ("small16", "two_wave", "first")
    return ("first", "loop") if case.family in ("stream", "stream16") else ("small", "loop")


def _bwd_cases():
    """(case, keys of derived_rows): W-split, node, plain and decoder shapes (three Linear layers) in every width class."""
    out = []
    for d, keys in ((128, ("bwd", "loop")), (100, ("two_wave", "bwd", "loop")), (48, ("loop",)), (20, ("loop",)), (200, ("loop",))):
        fam = "stream" if 64 < d <= 128 else "resident" if d <= 64 else "stream16"
        for shape in ("edge_wsplit", "node", "plain", "decoder"):
            out.append((Case(name=f"bwd_{shape}_{d}", family=fam, **_shape(shape, d)), keys))
    return tuple(out)


BWD_CASES = _bwd_cases()
BWD_BY_NAME = {c.name: c for c, _ in BWD_CASES}


# ------------------------------------------------------------------------------------------------ the generic kernel
ACT_PARAM = {"Tanh": 0.0, "Sigmoid": 0.0, "SiLU": 0.0, "GELU": 0.0, "LeakyReLU": 0.01, "ELU": 1.0}
GENERIC_WIDTH_CLASSES = ((20, 32), (48, 64), (100, 128), (200, 256))  # accumulator tiles WT = 1, 2, 4, 8
PADDED_WIDTHS = (20, 48, 100, 200)  # hidden lanes beyond the width carry act(0): 0.5 with Sigmoid


def generic_tiles(case: Case) -> tuple:
    """(HT, OT) of the mlp_fused_kernel instance that the dispatch switch of gnc_mlp_forward_f32 picks for a case."""
    tiles = lambda w: next(t for t in (1, 2, 4, 8) if w <= 32 * t)  # noqa: E731  (tiles_for, csrc/mlp_device.h)
    t, od = tiles(case.dims[0]), case.dims[-1]
    if od > 32:
        t = max(t, tiles(od))
    return (t, 1 if (od <= 32 and t > 1) else t)


def generic_lds_bytes(wt: int, layers: int) -> int:
    """lds_bytes(WT, L) of csrc/mlp_fused.hip: the weight chunk, the four waves' row tiles, the parameter rows."""
    return ((wt * 32 + 128) * 68 + (layers + 2) * wt * 32) * 4


def generic_loop_rows(cu: int, wt: int, layers: int = 3) -> int:
    """More 128-row tiles than the generic kernel's persistent grid has workgroups, the last tile ragged: the grid is
    CU x per_cu with per_cu = min(3, 160 KiB / lds_bytes(WT, L)), as in launch() of csrc/mlp_fused.hip."""
    per_cu = max(1, min(3, (160 * 1024) // generic_lds_bytes(wt, layers)))
    return 128 * cu * per_cu + 128 + 37


def _generic_cases():
    out = []

    def add(name, act, **kw):
        out.append(Case(name=name, family="generic", activation=act, act_param=ACT_PARAM.get(act, 0.0), **kw))

    # the model's launch shapes, six per width; every activation meets every width class, Sigmoid and GELU every padded width
    table = {
        20: (("plain", "Sigmoid"), ("edge_wsplit", "GELU"), ("node", "Tanh"), ("decoder", "SiLU"), ("concat_edge", "ELU"),
             ("encoder3", "LeakyReLU")),
        32: (("plain", "ELU"), ("edge_wsplit", "Sigmoid"), ("node", "LeakyReLU"), ("decoder5", "GELU"), ("concat_edge", "SiLU"),
             ("decoder", "Tanh")),
        48: (("plain", "GELU"), ("edge_wsplit", "Sigmoid"), ("node", "SiLU"), ("decoder", "ELU"), ("concat_edge", "Tanh"),
             ("decoder5", "LeakyReLU")),
        64: (("encoder3", "Tanh"), ("edge_wsplit", "ELU"), ("node", "GELU"), ("decoder", "Sigmoid"), ("concat_edge", "LeakyReLU"),
             ("plain", "SiLU")),
        100: (("plain", "Sigmoid"), ("edge_wsplit", "GELU"), ("node", "ELU"), ("decoder", "Tanh"), ("concat_edge", "SiLU"),
              ("encoder3", "LeakyReLU")),
        128: (("plain", "Tanh"), ("edge_wsplit", "SiLU"), ("node", "Sigmoid"), ("decoder", "GELU"), ("concat_edge", "ELU"),
              ("decoder5", "LeakyReLU")),
        200: (("plain", "GELU"), ("edge_wsplit", "Sigmoid"), ("node", "LeakyReLU"), ("decoder", "SiLU"), ("concat_edge", "Tanh"),
              ("encoder3", "ELU")),
        256: (("plain", "LeakyReLU"), ("edge_wsplit", "Tanh"), ("node", "SiLU"), ("decoder5", "ELU"), ("concat_edge", "GELU"),
              ("decoder", "Sigmoid")),
    }
    for d, pairs in table.items():
        for shape, act in pairs:
            add(f"generic_{shape}_{d}_{act}", act, **_shape(shape, d))
    add("generic_sliced_node_100_GELU", "GELU", **dict(_shape("node", 100), sliced=True))
    add("generic_nobias_100_Sigmoid", "Sigmoid", **_plain(100, (100, 100, 100), nobias=(0, 2)))
    add("generic_L2_48_SiLU", "SiLU", **_shape("plain", 48, layers=2))
    add("generic_L4_200_Tanh", "Tanh", **_shape("plain", 200, layers=4))
    # ReLU descriptions that every specialised kernel declines (the catch-all role).  A hidden width that is no multiple of 4
    # puts the second MATMUL segment of a [x | agg] launch on weight column 30 / 50 / 70 / 150: both streaming kernels want
    # wcol % 4 == 0.  The weights-resident kernel serves up to 64 features and a narrow output (<= 32) on plain shapes only;
    # the column-split kernel serves 65..128 features and a residual only with an output width that is a multiple of 4.
    for d in (30, 50):
        add(f"generic_relu_narrow_node_{d}_5", "ReLU", segs=((d, None, SEG_MATMUL), (d, None, SEG_MATMUL)), dims=(d, d, 5), ln=False)
    for d in (70, 150):
        add(f"generic_relu_node_{d}", "ReLU", **_shape("node", d))
    add("generic_relu_concat_edge_70", "ReLU", **_shape("concat_edge", 70))
    return tuple(out)


GENERIC_CASES = _generic_cases()
GENERIC_BY_NAME = {c.name: c for c in GENERIC_CASES}
assert len(GENERIC_BY_NAME) == len(GENERIC_CASES) and not set(GENERIC_BY_NAME) & set(BY_NAME)
# two shapes per width class also run with more tiles than the grid: wide-output and narrow-output instance where both exist
GENERIC_LOOP = ("generic_plain_20_Sigmoid", "generic_concat_edge_32_SiLU", "generic_edge_wsplit_48_Sigmoid", "generic_decoder_48_ELU",
                "generic_plain_100_Sigmoid", "generic_decoder_128_GELU", "generic_edge_wsplit_200_Sigmoid", "generic_decoder5_256_ELU")


def generic_rows(case: Case, small_batch_rows: int, cu: int) -> dict:
    """Row counts of a generic case by key: ``small`` for all, ``gloop`` for the cases of GENERIC_LOOP."""
    rows = {"small": derived_rows(small_batch_rows, cu)["small"]}
    if case.name in GENERIC_LOOP:
        rows["gloop"] = generic_loop_rows(cu, max(generic_tiles(case)), len(case.dims))
    return rows


def _generic_bwd_cases():
    """The backward through functional.fused_mlp (layer by layer on csrc/elementwise.hip): plain, node, concat_edge (gathered,
    shared table, residual) and decoder.  Widths 20, 48 and 200 are a width class each and run six activations (two shapes
    twice); 100 and 128 share theirs."""
    table = {
        20: (("plain", "Sigmoid"), ("node", "GELU"), ("concat_edge", "Tanh"), ("decoder", "SiLU"), ("plain", "LeakyReLU"), ("node", "ELU")),
        48: (("plain", "GELU"), ("node", "Sigmoid"), ("concat_edge", "LeakyReLU"), ("decoder", "ELU"), ("plain", "Tanh"), ("node", "SiLU")),
        100: (("plain", "GELU"), ("node", "Sigmoid"), ("concat_edge", "ELU"), ("decoder", "LeakyReLU")),
        128: (("plain", "SiLU"), ("node", "Tanh"), ("concat_edge", "Sigmoid"), ("decoder", "GELU")),
        200: (("plain", "Sigmoid"), ("node", "GELU"), ("concat_edge", "SiLU"), ("decoder", "Tanh"), ("plain", "ELU"), ("node", "LeakyReLU")),
    }
    return tuple(Case(name=f"gbwd_{shape}_{d}_{act}", family="generic", activation=act, act_param=ACT_PARAM[act], **_shape(shape, d))
                 for d, pairs in table.items() for shape, act in pairs)


GENERIC_BWD_CASES = _generic_bwd_cases()
GENERIC_BWD_BY_NAME = {c.name: c for c in GENERIC_BWD_CASES}
GENERIC_BWD_KEYS = ("small", "bwd")  # bwd = 64 x CU + 37 rows: more rows than layer_norm_backward_kernel has waves (16 blocks per
# CU x 4 waves), and at width >= 64 more elements than activation_kernel has threads (16 x 256 per CU)


# ------------------------------------------------------------------------------------------------ float64 definitions
def _D(x):
    return x.double().cpu()


def activate(z, activation: str = "ReLU", act_param: float = 0.0):
    """nn.<activation> in the dtype of ``z``: one torch.nn.functional call serves float64 and float32."""
    F = torch.nn.functional
    if activation == "ReLU":
        return torch.relu(z)
    if activation == "LeakyReLU":
        return F.leaky_relu(z, act_param)
    if activation == "ELU":
        return F.elu(z, act_param)
    return {"Tanh": torch.tanh, "Sigmoid": torch.sigmoid, "SiLU": F.silu, "GELU": F.gelu}[activation](z)


def forward_def(rows, modes, ws, bs, ln, residual, activation: str = "ReLU", act_param: float = 0.0):
    """The definition of gnc_mlp_forward_f32 on already gathered rows, in the dtype of its arguments (float64 for the
    reference, float32 for the host check): returns (out, hidden post-activations, hidden pre-activations, pre-LayerNorm)."""
    x = torch.cat([r for r, m in zip(rows, modes) if m == SEG_MATMUL], dim=1)
    z = x @ ws[0].t()
    if bs[0] is not None:
        z = z + bs[0]
    for r, m in zip(rows, modes):
        if m == SEG_ADD:
            z = z + r
    acts, pre = [], []
    for w, b in zip(ws[1:], bs[1:]):
        pre.append(z)
        z = activate(z, activation, act_param)
        acts.append(z)
        z = z @ w.t()
        if b is not None:
            z = z + b
    pre_ln = z
    if ln is not None:
        z = torch.nn.functional.layer_norm(z, (z.size(1),), ln[0], ln[1], ln[2])
    if residual is not None:
        z = z + residual
    return z, acts, pre, pre_ln


def _ref_forward(segs, modes, ws, bs, ln, residual):
    """float64 definition of gnc_mlp_forward_f32 on the tensors of a launch (host or device); returns (out, hidden
    post-activations)."""
    modes = modes or [SEG_MATMUL] * len(segs)
    rows = [(_D(tb) if ix is None else _D(tb)[ix.cpu().long()]) for tb, ix in segs]
    ln64 = (_D(ln[0]), _D(ln[1]), ln[2]) if ln is not None else None
    out, acts, _, _ = forward_def(rows, modes, [_D(w) for w in ws], [_D(b) if b is not None else None for b in bs], ln64,
                                  _D(residual) if residual is not None else None)
    return out, acts


# ------------------------------------------------------------------------------------------------ host inputs
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def view(op):
    """The operand itself: ``op`` = (wide tensor, first column, width)."""
    wide, off, w = op
    return wide if (off == 0 and w == wide.size(1)) else wide[:, off:off + w]


def to_device(op, dev):
    """The operand on the device, a column slice of the uploaded wide tensor where the case says so."""
    wide, off, w = op
    wide = wide.to(dev)
    return wide if (off == 0 and w == wide.size(1)) else wide[:, off:off + w]


def _operand(rng, r, c, sliced, draw):
    if not sliced:
        return (_f32(draw((r, c))), 0, c)
    wide = _f32(rng.standard_normal((r, c + 8)))  # the columns around the operand hold other values
    wide[:, 4:4 + c] = _f32(draw((r, c)))
    return (wide, 4, c)


def _inputs(case: Case, rows: int) -> dict:
    rng = np.random.default_rng(zlib.crc32(case.name.encode()) + rows)
    idx = {"src": torch.from_numpy(rng.integers(0, NODES, size=rows).astype(np.int32)),
           "dst": torch.from_numpy(np.sort(rng.integers(0, NODES, size=rows)).astype(np.int32))}
    c = {"case": case, "rows": rows, "index": idx, "pos": None}
    tables, shared = [], None
    for w, ix, _ in case.segs:
        if case.k6:
            from oracle import graphnet_oracle as O
            c["pos"] = _f32(rng.random((NODES, 2)) * 4)
            ei = torch.stack([idx["src"].long(), idx["dst"].long()])
            tables.append((O.edge_features(c["pos"], ei).contiguous(), 0, w))
        elif ix is not None and case.shared and shared is not None:
            tables.append(shared)
        else:
            tables.append(_operand(rng, rows if ix is None else NODES, w, case.sliced, rng.standard_normal))
            if ix is not None:
                shared = tables[-1]
    c["tables"] = tables
    ws, bs, i = [], [], case.in_dim
    for l, o in enumerate(case.dims):
        bound = 1.0 / np.sqrt(i)
        ws.append(_operand(rng, o, i, case.sliced, lambda s: rng.uniform(-bound, bound, s)))
        b = _f32(rng.uniform(-bound, bound, (o,)))
        bs.append(None if l in case.nobias else b)
        i = o
    c["ws"], c["bs"] = ws, bs
    od = case.dims[-1]
    c["ln"] = (_f32(rng.uniform(0.5, 1.5, od)), _f32(rng.uniform(-0.5, 0.5, od)), LN_EPS) if case.ln else None
    c["grad_out"] = _f32(rng.standard_normal((rows, od)))
    return c


def gathered_rows(c: dict, dtype):
    """Per segment the [rows, width] rows the launch reads, in ``dtype``."""
    return [view(op).to(dtype) if ix is None else view(op).to(dtype)[c["index"][ix].long()]
            for op, (_, ix, _) in zip(c["tables"], c["case"].segs)]


def evaluate(c: dict, dtype):
    """forward_def of the case on its host inputs in ``dtype``."""
    case = c["case"]
    rows = gathered_rows(c, dtype)
    ln = (c["ln"][0].to(dtype), c["ln"][1].to(dtype), c["ln"][2]) if c["ln"] is not None else None
    return forward_def(rows, case.modes, [view(w).to(dtype) for w in c["ws"]],
                       [b.to(dtype) if b is not None else None for b in c["bs"]], ln,
                       rows[case.res] if case.res is not None else None, case.activation, case.act_param)


def _case_of(name: str) -> Case:
    for table in (BY_NAME, BWD_BY_NAME, GENERIC_BY_NAME, GENERIC_BWD_BY_NAME):
        if name in table:
            return table[name]
    raise KeyError(name)


@functools.lru_cache(maxsize=2)
def build(name: str, rows: int) -> dict:
    """Host inputs and the float64 forward of a case: ``out``, ``acts``, ``pre`` (hidden pre-activations), ``pre_ln``."""
    c = _inputs(_case_of(name), rows)
    with torch.no_grad():
        c["out"], c["acts"], c["pre"], c["pre_ln"] = evaluate(c, torch.float64)
    c["bar"] = TOL * max(1.0, float(c["out"].abs().max()))
    return c


def autograd(c: dict, dtype, grad_out) -> dict:
    """Autograd of the case's definition in ``dtype``: ``dz0`` (gradient of the first pre-activation = of both gathered ADD
    rows), ``dx`` (gradient of the concatenated row-ordered MATMUL rows, residual path INCLUDED), ``dw`` / ``db`` per Linear,
    ``dbeta`` / ``dgamma``."""
    case = c["case"]
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)  # noqa: E731  (the case's own tensors stay as they are)
    rows = [leaf(r) for r in gathered_rows(c, dtype)]
    ws = [leaf(view(w)) for w in c["ws"]]
    bs = [leaf(b) if b is not None else None for b in c["bs"]]
    ln = (leaf(c["ln"][0]), leaf(c["ln"][1]), c["ln"][2]) if c["ln"] else None
    out, _, pre, pre_ln = forward_def(rows, case.modes, ws, bs, ln, rows[case.res] if case.res is not None else None,
                                      case.activation, case.act_param)
    z0 = pre[0] if pre else pre_ln
    z0.retain_grad()
    out.backward(grad_out.to(dtype))
    return {"dz0": z0.grad, "dx": torch.cat([r.grad for r, m in zip(rows, case.modes) if m == SEG_MATMUL], dim=1),
            "dw": [w.grad for w in ws], "db": [b.grad if b is not None else None for b in bs],
            "dgamma": ln[0].grad if ln else None, "dbeta": ln[1].grad if ln else None}


def table_gradients(c: dict, grads: dict, grad_out) -> list:
    """Per segment the gradient of its TABLE from ``grads`` (of ``autograd``), in the dtype of ``grads``: the rows of ``dx`` for
    a row-ordered segment, summed per table row for a gathered one (over both segments where they share a table: those entries
    are one tensor).  The residual path is taken out of its segment: it belongs to the residual's own gradient, ``grad_out``."""
    case, out, by_table, off = c["case"], [], {}, 0
    for s, (w, ix, _) in enumerate(case.segs):
        g = grads["dx"][:, off:off + w].clone()
        off += w
        if s == case.res:
            g -= grad_out.to(g.dtype)
        if ix is not None:
            g = torch.zeros(NODES, w, dtype=g.dtype).index_add_(0, c["index"][ix].long(), g)
            key = id(c["tables"][s][0])
            if key in by_table:
                by_table[key] += g
                g = by_table[key]
            by_table[key] = g
        out.append(g)
    return out


@functools.lru_cache(maxsize=2)
def build_backward(name: str, rows: int) -> dict:
    """``build`` + ``marked`` (rows with a hidden pre-activation within KINK of zero in float64; none for an activation without
    a kink), ``grad_out`` with those rows zeroed, and float64 autograd on it (``grads``)."""
    c = dict(build(name, rows))
    marked = torch.zeros(rows, dtype=torch.bool)
    for z in c["pre"] if c["case"].activation in KINKED else ():
        marked |= (z.abs() < KINK).any(dim=1)
    g = c["grad_out"].clone()
    g[marked] = 0.0
    c["marked"], c["grad_out"] = marked, g
    c["marked_share"] = float(marked.float().mean())
    c["grads"] = autograd(c, torch.float64, g)
    return c
