"""GPU: the three per-graph pooling families - global pooling (K17), attention read-out (K19), top-K pooling (K20) - give the bits
they gave BEFORE their kernels moved onto one reduction skeleton (csrc/graph_reduce.h) and one set of row helpers.

The fixtures under tests/golden/pool_family_bits/ were recorded from the library of the parent commit by
tests/golden/make_pool_family_bits_golden.py (its JSON names that commit); this module replays the same seeded cases on the
library under test and asserts equality of every byte.  Per-graph tensors (``out``, ``argmax``, ``saved``), ``alpha`` and ``ds``
are stored whole; every [rows, C] tensor is stored as shape and SHA-256.

Batches, with R = the plan's ``chunk_rows``, at widths 1, 3, 64 and 130:
  many        graphs of 0, 1, 63, 64, 65, R, R + 1, 2R + 37 and 5 rows and 40 slack rows (the many-graphs regime)
  split-1     the 2R + 37 graph alone (the split regime)
  split-3     7 rows in front of graph_ptr[0], graphs of 5R + 3, 0 and 2R rows, 40 slack rows (the split regime, three graphs)
  misaligned  ``many`` at widths 64 and 130 with y starting 4 bytes past a 16-byte boundary (the scalar path of the VEC = 4 kernels)
K20 runs the sizes of tests/topk_pool_cases.py up to 257 rows as one batch through select, edge filter and the row launches."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_family_bits")
WIDTHS = (1, 3, 64, 130)
BATCHES = ("many", "split-1", "split-3", "misaligned")
KEYS = [(family, batch) for family in ("k17", "k19") for batch in BATCHES] + [("k20", "small")]


def sha256(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()


def batch_of(native, name):
    """``(graph_ptr int64 [G + 1], rows, widths, expected split, misaligned)``."""
    R = native.graph_pool_plan(1000, 64, 9)["chunk_rows"]
    front, sizes, slack = {"many": (0, [0, 1, 63, 64, 65, R, R + 1, 2 * R + 37, 5], 40), "split-1": (0, [2 * R + 37], 0),
                           "split-3": (7, [5 * R + 3, 0, 2 * R], 40), "misaligned": (0, [0, 1, 63, 64, 65, R, R + 1, 2 * R + 37, 5], 40)}[name]
    gp = torch.tensor([front] + sizes).cumsum(0)
    rows = int(gp[-1]) + slack
    widths = (64, 130) if name == "misaligned" else WIDTHS
    split = 0 if name in ("many", "misaligned") else 1
    for C in widths:
        assert native.graph_pool_plan(rows, C, len(sizes))["split"] == split, (name, C)
    return gp, rows, widths, split, name == "misaligned"


def on_device(t, misaligned):
    """``t`` on the device; ``misaligned``: as a contiguous view one float into a larger buffer."""
    if not misaligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def run_k17(native, batch):
    gp, rows, widths, _, mis = batch_of(native, batch)
    G = gp.numel() - 1
    gen = torch.Generator().manual_seed(1700 + BATCHES.index(batch))
    whole, hashed = {}, {}
    for C in widths:
        base = torch.randn(rows, C, generator=gen)
        ties = torch.round(base * 2) / 2  # values rounded to halves: ties of the maximum, and a few special cells
        cells = torch.randint(0, rows * C, (9,), generator=gen)
        ties.view(-1)[cells] = torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat(3)
        for kind, y in (("randn", base), ("ties", ties)):
            y_dev = on_device(y, mis)
            for mode, bits in native.POOL_MODES.items():
                out, argmax = native.graph_pool_forward(y_dev, gp.to(DEV), bits)
                grad = torch.randn(G, out.size(1), generator=gen)
                dy = native.graph_pool_backward(grad.to(DEV), bits, argmax, gp.to(DEV), rows)
                torch.cuda.synchronize()
                key = f"{C}/{kind}/{mode}"
                whole[key + "/out"] = out.cpu()
                if argmax is not None:
                    whole[key + "/argmax"] = argmax.cpu()
                hashed[key + "/dy"] = dy.cpu()
    return whole, hashed


def run_k19(native, batch):
    gp, rows, widths, _, mis = batch_of(native, batch)
    G = gp.numel() - 1
    gen = torch.Generator().manual_seed(1900 + BATCHES.index(batch))
    whole, hashed = {}, {}
    for C in widths:
        y = on_device(torch.randn(rows, C, generator=gen), mis)
        unit = torch.randn(rows, generator=gen)
        grad = torch.randn(G, C, generator=gen).to(DEV)
        for kind, scale in (("narrow", 4.0), ("wide", 200.0)):
            scores = (scale * unit).to(DEV)
            out, saved = native.graph_attention_pool_forward(y, scores, gp.to(DEV))
            alpha = native.graph_attention_weights(scores, saved, gp.to(DEV))
            dy, ds = native.graph_attention_pool_backward(grad, y, scores, out, saved, gp.to(DEV))
            dy_alone, _ = native.graph_attention_pool_backward(grad, y, scores, out, saved, gp.to(DEV), need_ds=False)
            _, ds_alone = native.graph_attention_pool_backward(grad, y, scores, out, saved, gp.to(DEV), need_dy=False)
            torch.cuda.synchronize()
            key = f"{C}/{kind}"
            whole.update({key + "/out": out.cpu(), key + "/saved": saved.cpu(), key + "/alpha": alpha.cpu(), key + "/ds": ds.cpu(),
                          key + "/ds_alone": ds_alone.cpu()})
            hashed.update({key + "/dy": dy.cpu(), key + "/dy_alone": dy_alone.cpu()})
    return whole, hashed


def run_k20(native, batch):
    from tests import topk_pool_cases as K
    sizes = [n for n in K.SIZES if n <= 257]
    rng = np.random.default_rng(2000)
    gp = torch.tensor([5] + sizes).cumsum(0)
    rows = int(gp[-1]) + 9
    whole, hashed = {}, {}
    patterns = K.score_patterns(rng, rows)
    src, dst, rowptr = K.sorted_edges(rng, rows, K.EDGE_TILE + 1, hub=True)
    for kind in ("duplicates", "special"):
        scores = torch.from_numpy(patterns[kind]).to(DEV)
        new_id, kept, gp_out, counts = native.topk_pool_select(scores, gp.to(DEV), 0.5)
        edges = native.topk_pool_filter_edges(torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV), torch.from_numpy(rowptr).to(DEV),
                                              new_id, kept, counts)
        n_out, e_out = (int(v) for v in counts.cpu())
        whole.update({kind + "/new_id": new_id.cpu(), kind + "/kept": kept[:n_out].cpu(), kind + "/graph_ptr": gp_out.cpu(),
                      kind + "/counts": counts.cpu(), kind + "/edge_new_id": edges[3].cpu(), kind + "/rowptr": edges[4][:n_out + 1].cpu()})
        for name, t in zip(("src", "dst", "kept_edges"), edges[:3]):
            whole[f"{kind}/{name}"] = t[:e_out].cpu()
        gate_scores = torch.from_numpy(patterns["random"]).to(DEV)
        for C in (3, 64):
            x = torch.from_numpy(rng.standard_normal((rows, C)).astype(np.float32)).to(DEV)
            grad = torch.from_numpy(rng.standard_normal((n_out, C)).astype(np.float32)).to(DEV)
            for gate in (None, gate_scores):
                out = native.topk_pool_rows_forward(x, kept[:n_out], gate)
                dx, ds = native.topk_pool_rows_backward(grad, new_id, x, gate)
                torch.cuda.synchronize()
                key = f"{kind}/{C}/{'gate' if gate is not None else 'plain'}"
                hashed.update({key + "/out": out.cpu(), key + "/dx": dx.cpu()})
                if ds is not None:
                    whole[key + "/ds"] = ds.cpu()
    return whole, hashed


def run_case(native, family, batch):
    """``(whole, hashed)``: name -> CPU tensor, for the tensors the fixture keeps whole and those it keeps as shape and SHA-256."""
    return {"k17": run_k17, "k19": run_k19, "k20": run_k20}[family](native, batch)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "pool_family_bits.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "pool_family_bits.npz"))


def test_the_fixtures_name_the_commit_they_were_recorded_from(golden):
    meta, arrays = golden
    assert len(meta["commit"]) == 40 and meta["library"] != "graphnet_classifier_amd/libgnc_hip.so"
    assert sorted(meta["cases"]) == sorted(f"{f}/{b}" for f, b in KEYS)
    assert sorted(arrays.files) == sorted(f"{case}/{k}" for case, c in meta["cases"].items() for k in c["whole"])


@pytest.mark.parametrize("family,batch", KEYS)
def test_every_byte_is_the_parents(golden, family, batch):
    from graphnet_classifier_amd import native
    native.load_library()
    meta, arrays = golden
    case = meta["cases"][f"{family}/{batch}"]
    whole, hashed = run_case(native, family, batch)
    assert sorted(whole) == sorted(case["whole"]) and sorted(hashed) == sorted(case["hashed"])
    for k, t in whole.items():
        want = arrays[f"{family}/{batch}/{k}"]
        got = t.numpy()
        assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes(), (family, batch, k)
    for k, t in hashed.items():
        assert list(t.shape) == case["hashed"][k]["shape"] and sha256(t) == case["hashed"][k]["sha256"], (family, batch, k)
