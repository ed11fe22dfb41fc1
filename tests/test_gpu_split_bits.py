"""The split class of the weights-resident MLP kernel (3-way bf16 split on the bf16 matrix pipe), bit for bit.

1. Against fixtures recorded from the PARENT of the commit that re-expressed the split (tests/golden/split_bits/, written by
   tests/golden/make_split_bits_golden.py with the parent's library selected through GNC_LIB_PATH; split_bits.json names the
   commit): the whole flagship forward at 1/25 of c3 (250 graphs, 40,000 nodes, 400,000 edges - every launch shape of the
   forward is then served by the resident split class: EF encoder, DUAL projection, storing and aggregate-only edge processor,
   node processors, decoder), and the two native.mlp_forward launches of tests/test_gpu_split_mlp.py (70,007 rows: a wave
   walks more than one tile), the latter as SHA-256 of the output bytes plus every 97th row.

2. A property that needs no fixture: the single-Linear projection (split class 1) with a signed permutation matrix scaled by
   powers of two.  Every MFMA sum then has one non-zero term, and the three planes of an input add up to the input exactly, so
   the output is known bit for bit whatever order the matrix pipe adds in."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_split_mlp as split_mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "split_bits")
DEV = "cuda"

pytestmark = pytest.mark.gpu


def _meta():
    with open(os.path.join(GOLDEN, "split_bits.json")) as f:
        return json.load(f)


def test_flagship_forward_bits_match_parent():
    from graphnet_classifier_amd import native, synthetic
    from graphnet_classifier_amd.GNN import GraphNet
    from graphnet_classifier_amd.topology import clear_topology_cache
    native.load_library()
    meta = _meta()["graphnet"]
    want = torch.from_numpy(np.load(os.path.join(GOLDEN, "graphnet_c3_004.npy")))
    batch, kw = synthetic.make_workload(meta["workload"], meta["scale"])
    assert (batch.num_graphs, batch.num_nodes, batch.num_edges) == (250, 40000, 400000)
    torch.manual_seed(0)
    model = GraphNet(**kw).to(DEV).eval()
    clear_topology_cache()
    with torch.no_grad():
        y = model(batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV))
    torch.cuda.synchronize()
    y = y.cpu()
    assert y.shape == want.shape == (40000, 1) and y.dtype == want.dtype == torch.float32
    differ = int((y.view(torch.int32) != want.view(torch.int32)).sum())
    print(f"flagship forward at c3 x 0.04: {differ} of {y.numel()} outputs differ from the parent's, "
          f"max abs difference {float((y - want).abs().max()):.3e}")
    assert torch.equal(y, want)


@pytest.mark.parametrize("kind", ["edge", "enc"])
def test_mlp_forward_bits_match_parent(kind):
    from graphnet_classifier_amd import native
    native.load_library()
    meta = _meta()
    step = meta["row_step"]
    want_rows = torch.from_numpy(np.load(os.path.join(GOLDEN, f"mlp_{kind}_rows.npy")))
    out, _ = split_mlp._forward(native, kind, split_mlp._case(kind))
    assert list(out.shape) == meta["mlp"][kind]["shape"] and out.shape[0] == split_mlp.ROWS
    rows = out[::step]
    differ = int((rows.view(torch.int32) != want_rows.view(torch.int32)).sum())
    digest = hashlib.sha256(np.ascontiguousarray(out.numpy()).tobytes()).hexdigest()
    print(f"{kind}: {differ} of {rows.numel()} sampled values differ from the parent's; sha256 {digest} "
          f"(parent {meta['mlp'][kind]['sha256']})")
    assert torch.equal(rows, want_rows)
    assert digest == meta["mlp"][kind]["sha256"]


# ---- the property test ------------------------------------------------------------------------------------------------
P_ROWS, P_W = 33000, 64  # just above the rows the small-batch kernel serves: the resident kernel, single-Linear projection


def _split_inputs():
    """[P_ROWS, 64] fp32: random signs and mantissas over the 60 binades 2^-30 .. 2^29, a quarter of them exactly halfway
    between two bf16 neighbours (low 16 bits 0x8000: the first rounding is a tie), others one ulp to either side of such a
    tie, some with no bits below bf16 at all, and +0 / -0."""
    g = torch.Generator().manual_seed(20)
    n = P_ROWS * P_W
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64) << 31
    expo = torch.randint(127 - 30, 127 + 30, (n,), generator=g, dtype=torch.int64) << 23
    mant = torch.randint(0, 1 << 23, (n,), generator=g, dtype=torch.int64)
    kind = torch.randint(0, 16, (n,), generator=g, dtype=torch.int64)
    hi = mant & ~0xffff
    mant = torch.where(kind < 4, hi | 0x8000, mant)    # exact ties
    mant = torch.where(kind == 4, hi | 0x7fff, mant)   # just below a tie
    mant = torch.where(kind == 5, hi | 0x8001, mant)   # just above
    mant = torch.where(kind == 6, hi, mant)            # a bf16 value
    mant = torch.where(kind == 7, (mant & ~0xff) | 0x80, mant)  # a tie of the second rounding
    bits = sign | expo | mant
    bits = torch.where(kind == 8, sign, bits)          # +0 / -0
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    return bits.view(torch.float32).reshape(P_ROWS, P_W)


def _planes_add_up(x):
    """bf16(x) + bf16(x - x0) + bf16(x - x0 - x1) == x with torch's round-to-nearest-even bfloat16 (every term exact in fp64)."""
    x0 = x.bfloat16().float()
    r1 = x - x0
    x1 = r1.bfloat16().float()
    r2 = r1 - x1
    x2 = r2.bfloat16().float()
    assert torch.equal(r1.double(), x.double() - x0.double()) and torch.equal(r2.double(), r1.double() - x1.double())
    return (x0.double() + x1.double() + x2.double()) == x.double()


def test_split_projection_signed_permutation_is_exact():
    from graphnet_classifier_amd import native
    native.load_library()
    x = _split_inputs()
    ok = _planes_add_up(x)
    dropped = int((~ok).sum())
    print(f"inputs whose three planes do not add up (replaced by 1.0): {dropped} of {x.numel()}")
    assert dropped <= 0.01 * x.numel()
    x = torch.where(ok, x, torch.ones_like(x))
    expo = torch.frexp(x[x != 0].abs())[1]
    assert int(expo.max()) - int(expo.min()) + 1 >= 60  # binades covered
    assert bool(((x == 0) & torch.signbit(x)).any()) and bool(((x == 0) & ~torch.signbit(x)).any())

    g = torch.Generator().manual_seed(21)
    perm = torch.randperm(P_W, generator=g)
    scale = torch.ldexp(torch.ones(P_W), torch.randint(-8, 9, (P_W,), generator=g)) * (1.0 - 2.0 * torch.randint(0, 2, (P_W,), generator=g))
    w = torch.zeros(P_W, P_W)
    w[torch.arange(P_W), perm] = scale  # out[:, n] = scale[n] * x[:, perm[n]]
    out = native.mlp_forward([(x.to(DEV), None)], [w.to(DEV)], [None])
    torch.cuda.synchronize()
    out = out.cpu()
    # the accumulator starts at +0 (no bias) and every other term of the sums is a zero: 0 + s x, exact, and +0 where x is -0
    want = torch.zeros(P_ROWS, P_W) + x[:, perm] * scale
    assert torch.equal(want.double(), 0.0 + x[:, perm].double() * scale.double())  # the expectation itself is exact in fp32
    differ = int((out.view(torch.int32) != want.view(torch.int32)).sum())
    print(f"signed permutation projection: {differ} of {out.numel()} outputs differ in their bits")
    assert out.shape == want.shape
    assert differ == 0
