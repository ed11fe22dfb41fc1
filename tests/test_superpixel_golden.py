"""CPU checks of the SLIC superpixel fixtures (tests/golden/g10_superpixel*.npz, captured from scikit-image 0.18.3
and the reference's own image_to_graph_superpixel by tests/golden/make_superpixel_golden.py) and of the ABI that
carries the device SLIC (csrc/superpixel.hip)."""
import numpy as np
import pytest

from oracle import image_graph_oracle as IO
from tests._util import load_golden


def superpixel_cases():
    """(case id, image, labels, (n_segments, compactness, max_iter, enforce_connectivity), graph or None)."""
    out = []
    for name in ("g10_superpixel.npz", "g10_superpixel_256.npz"):
        g = load_golden(name)
        out.append(g)
    small, big = out
    params = small["params"]
    cases = []
    for i, (n, c, mi, ec, has_graph) in enumerate(params):
        d = big if f"img_{i}" in big else small
        graph = (d[f"graph_x_{i}"], d[f"graph_pos_{i}"], d[f"graph_ei_{i}"]) if has_graph else None
        cases.append((i, d[f"img_{i}"], d[f"labels_{i}"], (int(n), float(c), int(mi), bool(ec)), graph))
    return cases


CASES = superpixel_cases()


def test_fixture_covers_what_the_device_slic_must_reproduce():
    g = load_golden("g10_superpixel.npz")
    assert tuple(g["versions"])[0] == "0.18.3"
    shapes = {img.shape[:2] for _, img, _, _, _ in CASES}
    assert {(32, 32), (64, 64), (128, 128), (256, 256), (96, 160)} <= shapes
    opts = {p for _, _, _, p, _ in CASES}
    assert (100, 10.0, 10, False) in opts and (100, 10.0, 1, True) in opts and (100, 10.0, 1, False) in opts
    assert {25, 400} <= {p[0] for p in opts} and {1.0, 30.0} <= {p[1] for p in opts}
    assert g["merge"].any() and g["capped"].any()  # a small-component merge and a max_size-capped flood fill
    assert sum(graph is not None for *_, graph in CASES) == 26
    for _, img, labels, _, _ in CASES:
        assert img.dtype == np.uint8 and labels.dtype == np.int32 and labels.shape == img.shape[:2]


@pytest.mark.parametrize("case", [c for c in CASES if c[4] is not None], ids=lambda c: f"case{c[0]}")
def test_oracle_superpixel_graph_pinned_to_reference(case):
    _, img, labels, _, (rx, rpos, rei) = case
    x, pos, ei = IO.superpixel_graph_from_labels(img, labels)
    assert np.array_equal(np.asarray(ei, dtype=np.int64), rei)
    assert np.array_equal(np.asarray(x, dtype=np.float32), rx)
    assert np.array_equal(np.asarray(pos, dtype=np.float32), rpos)


def test_slic_symbols_exported_at_abi_20():
    from graphnet_classifier_amd import native
    lib = native.load_library()
    assert lib.gnc_abi_version() == 20
    for name in ("gnc_slic_workspace_bytes", "gnc_slic_rgb_u8"):
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.gnc_slic_workspace_bytes(2, 128, 128, 100) > 2 * 128 * 128 * 24
    assert lib.gnc_slic_workspace_bytes(1, 0, 128, 100) == 0
    assert lib.gnc_slic_workspace_bytes(1, 128, 128, 0) == 0
