"""Descriptions for the fused-MLP routing table (tests/golden/mlp_routes.json, tests/test_mlp_routes_host.py).

A deterministic enumeration of gnc_mlp_desc_t / gnc_mlp_bwd_desc_t values with fake 16-B aligned addresses (the shape
queries never dereference them, and answer without a GPU), and the 14 queries whose answers make up the table.  The
recorder (tests/golden/make_mlp_routes_golden.py) and the test walk the same enumeration, so a case is its position in it.

Run as a program this prints the answer table of the loaded library as JSON: that is how the A/B switches, each read once
per process, are recorded and replayed (one fresh child per switch)."""
import array
import base64
import ctypes
import itertools
import json
import sys
import zlib

FAKE = 0x10000        # never dereferenced; 16-B aligned
STEP = 0x1000000      # distance between two fake tensors

FORMS = ("table", "table_in3", "table_out3", "mm2_rows", "mm2_gather", "mm3_rows", "mm3_gather", "wsplit", "ef_pos")
WIDTHS = (3, 20, 32, 48, 64, 100, 128, 200, 256)
LAYERS = (1, 2, 3, 4)
LN = (False, True)

# residual, other activation, ld not a multiple of 4, fwd.save_act, act_given, dx wanted, dw_partial, grad_gather (0 none, 1 with
# the index of seg[2], 2 with another index)
VARIANTS = (
    (0, 0, 0, 0, 0, 1, 0, 0),
    (1, 0, 0, 1, 1, 1, 0, 0),
    (1, 0, 0, 1, 1, 1, 1, 1),
    (0, 0, 0, 1, 1, 0, 1, 2),
    (1, 0, 0, 0, 0, 1, 1, 1),
    (1, 1, 0, 0, 0, 1, 0, 0),
    (1, 0, 1, 1, 1, 1, 0, 0),
    (0, 0, 1, 0, 0, 0, 0, 0),
    (0, 0, 0, 1, 1, 0, 0, 1),
    (1, 0, 0, 1, 0, 1, 0, 2),
    (0, 0, 0, 0, 1, 1, 0, 0),
    (0, 1, 0, 1, 1, 1, 1, 0),
)

# (name, which description it takes, True: the answer is a return code compared as zero / nonzero)
QUERIES = (
    ("gnc_mlp_supported", "fwd", True),
    ("gnc_mlp_agg_supported", "fwd", True),
    ("gnc_mlp_agg_only_supported", "fwd", True),
    ("gnc_mlp_save_act_supported", "fwd", True),
    ("gnc_mlp_operands_in_place_supported", "fwd", True),
    ("gnc_mlp_edge_features_supported", "fwd", True),
    ("gnc_mlp_small_batch_supported", "fwd", True),
    ("gnc_mlp_backward_supported", "fwd", True),
    ("gnc_mlp_backward_small_batch_supported", "fwd", False),
    ("gnc_mlp_backward_dx_add_honoured", "fwd", False),
    ("gnc_mlp_backward_saved_act_honoured", "bwd", False),
    ("gnc_mlp_backward_grad_gather_honoured", "bwd", False),
    ("gnc_mlp_backward_fused_rows", "fwd", False),
    ("gnc_mlp_backward_ln_partial_rows", "fwd", False),
)

# A/B switches of the two routers: each is read once per process, so each gets a child process and a thinned grid
SWITCHES = ("GNC_NO_BACKWARD16", "GNC_NO_STREAM_DX_FOLD", "GNC_NO_SAVED_ACT", "GNC_NO_GRAD_GATHER_FOLD", "GNC_NO_FUSED_BACKWARD",
            "GNC_NO_STREAM_LN_SUMS", "GNC_STREAM16_D128", "GNC_NO_SMALL16")
SWITCH_STRIDE = 7     # the switch grids take every 7th case (coprime to the number of variants: every variant is met)


def row_counts(lib):
    small = int(lib.gnc_mlp_small_batch_max_rows())
    return (0, 1, 777, small, small + 1, 40_003, 65_829, 10_000_000)


def _addr(k):
    return FAKE + k * STEP


def describe(native, form, width, layers, rows, ln, variant):
    """One backward description (its ``fwd`` member is the forward one), in the segment order the binding hands to the kernels."""
    res, other_act, odd_ld, save, given, dx, dwp, gg = variant
    bd = native.MlpBwdDesc()
    d = bd.fwd
    out_w = 3 if form == "table_out3" else width
    seg_w = 3 if form in ("table_in3", "ef_pos") else width
    n_mm = {"mm2_rows": 2, "mm2_gather": 2, "mm3_rows": 3, "mm3_gather": 3}.get(form, 1)
    n_add = 2 if form == "wsplit" else 0
    ld_pad = 1 if odd_ld else 0
    d.num_segments, d.num_linear = n_mm + n_add, layers
    d.activation = native.ACTIVATIONS["ELU"] if other_act else native.ACTIVATIONS["ReLU"]
    d.act_param = 1.0 if other_act else 0.0
    for s in range(n_mm + n_add):
        g = d.seg[s]
        g.ptr, g.width, g.ld = _addr(1 + s), seg_w, seg_w + ld_pad
        if s < n_mm:
            g.mode, g.wcol = native.SEG_MATMUL, s * seg_w
            gathered = form.endswith("_gather") and s < n_mm - 1   # the row-ordered (residual) segment comes last
        else:
            g.mode, g.width, g.ld, gathered = native.SEG_ADD, width, width + ld_pad, True
        if gathered:
            g.index, g.table_rows = _addr(8 + s), 1_000_000
    if form == "ef_pos":
        d.seg[0].ld = 4
        d.ef_pos, d.ef_src, d.ef_dst, d.ef_nodes, d.ef_space_dim = _addr(12), _addr(13), _addr(14), 1_000_000, 2
    for l in range(layers):
        d.in_dim[l] = n_mm * seg_w if l == 0 else width
        d.out_dim[l] = out_w if l == layers - 1 else width
        d.weight[l], d.bias[l] = _addr(16 + l), _addr(24 + l)
        d.ld_weight[l] = d.in_dim[l] + ld_pad
    if ln:
        d.ln_gamma, d.ln_beta, d.ln_eps = _addr(32), _addr(33), 1e-5
    if res:  # the last MATMUL segment when it is row-ordered and as wide as the output, else a tensor of its own
        last = d.seg[n_mm - 1]
        d.residual = last.ptr if (seg_w == out_w and not last.index) else _addr(34)
        d.ld_residual = last.ld if d.residual == last.ptr else out_w
    d.out, d.ld_out, d.rows = _addr(35), out_w, rows
    for l in range(layers - 1):
        if save:
            d.save_act[l] = _addr(40 + l)
        if given:
            bd.act[l] = _addr(40 + l)
    bd.act_given = given
    bd.grad_out, bd.ld_grad_out = _addr(48), out_w + ld_pad
    if dx:
        bd.dx, bd.ld_dx = _addr(49), d.in_dim[0]
    bd.dx_add_grad_out = res
    if dwp:
        for l in range(layers):
            bd.dw_partial[l] = _addr(50 + l)
    if gg:
        bd.grad_gather, bd.ld_grad_gather = _addr(58), out_w + ld_pad
        same = gg == 1 and d.num_segments == 3
        bd.grad_gather_index = d.seg[2].index if same and d.seg[2].index else _addr(59)
        bd.grad_gather_rows = d.seg[2].table_rows if same else 500_000
    return bd


def invalid(native):
    """A few descriptions that gnc_mlp_supported must refuse."""
    v = VARIANTS[1]
    out = []
    bd = describe(native, "table", 64, 3, 777, True, v)
    bd.fwd.num_linear = 0
    out.append(bd)
    bd = describe(native, "mm2_rows", 64, 3, 777, True, v)
    bd.fwd.in_dim[0] = 100                       # segment widths do not sum to it
    out.append(bd)
    bd = describe(native, "table", 64, 3, 777, True, v)
    bd.fwd.activation = 99
    out.append(bd)
    bd = describe(native, "table", 64, 4, 777, True, v)
    bd.fwd.out_dim[1], bd.fwd.in_dim[2] = 32, 32  # hidden layers of two widths
    out.append(bd)
    bd = describe(native, "wsplit", 64, 3, 65_829, True, v)
    bd.fwd.seg[1].width = 48                     # additive segment narrower than the first Linear
    out.append(bd)
    bd = describe(native, "table", 64, 3, 777, True, v)
    bd.fwd.rows = -1
    out.append(bd)
    bd = describe(native, "table", 64, 2, 777, False, v)
    bd.fwd.out_dim[0], bd.fwd.in_dim[1] = 300, 300
    out.append(bd)
    return out


def cases(native, lib, stride=1):
    """Every ``stride``-th description of the grid, then (stride 1 only) the invalid ones."""
    grid = itertools.product(FORMS, WIDTHS, LAYERS, row_counts(lib), LN, VARIANTS)
    for p in itertools.islice(grid, 0, None, stride):
        yield describe(native, *p)
    if stride == 1:
        yield from invalid(native)


def answers(native, lib, stride=1):
    """(distinct answer vectors in order of first appearance, index of each case's vector)."""
    fns = [(getattr(lib, name), which == "fwd", is_rc) for name, which, is_rc in QUERIES]
    vectors, index, seen = [], [], {}
    for bd in cases(native, lib, stride):
        fwd, whole = ctypes.byref(bd.fwd), ctypes.byref(bd)
        vec = []
        for fn, takes_fwd, is_rc in fns:
            a = int(fn(fwd if takes_fwd else whole))
            vec.append((1 if a else 0) if is_rc else a)
        vec = tuple(vec)
        if vec not in seen:
            seen[vec] = len(vectors)
            vectors.append(list(vec))
        index.append(seen[vec])
    return vectors, index


def pack(tables):
    """{name: {"vectors", "index"}} as the golden file stores it: the distinct answer vectors of all tables once, and per table
    one uint16 per case (its vector's position in that list), deflated, in base64."""
    shared, stored = {}, {}
    for name, t in tables.items():
        ids = array.array("H", (shared.setdefault(tuple(t["vectors"][k]), len(shared)) for k in t["index"]))
        if sys.byteorder == "big":
            ids.byteswap()
        stored[name] = {"cases": len(ids), "index_u16le_zlib_b64": base64.b64encode(zlib.compress(ids.tobytes(), 9)).decode("ascii")}
    return {"vectors": [list(v) for v in shared], "tables": stored}


def unpack(stored):
    tables = {}
    for name, t in stored["tables"].items():
        ids = array.array("H", zlib.decompress(base64.b64decode(t["index_u16le_zlib_b64"])))
        if sys.byteorder == "big":
            ids.byteswap()
        assert len(ids) == t["cases"]
        tables[name] = {"vectors": stored["vectors"], "index": list(ids)}
    return tables


if __name__ == "__main__":  # child of the recorder / the test: the environment carries the switch
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from graphnet_classifier_amd import native as _native
    _vectors, _index = answers(_native, _native.load_library(), int(sys.argv[1]))
    json.dump({"vectors": _vectors, "index": _index}, sys.stdout)
