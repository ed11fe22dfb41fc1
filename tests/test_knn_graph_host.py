"""Host: the C ABI of the k-nearest-neighbour kernel (K24) - symbols, header, the supported set decided before any HIP call -
the Python-side argument errors, and the NumPy reference's self-checks.  No GPU is needed."""
import os
import re

import numpy as np
import pytest
import torch

from graphnet_classifier_amd import functional as F
from graphnet_classifier_amd import image_to_graph as I2G
from graphnet_classifier_amd import native
from tests import knn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GNC_ERR_UNSUPPORTED = -2


def test_symbols_header_and_abi():
    lib = native.load_library()
    header = open(os.path.join(ROOT, "include", "gnc_hip.h")).read()
    for name in ("gnc_knn_graph_f32", "gnc_knn_graph_padded_f32"):
        assert hasattr(lib, name) and name in native.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert lib.gnc_abi_version() == native.ABI_VERSION == 20
    assert re.search(r"#define\s+GNC_ABI_VERSION\s+20\b", header)
    q, unroll = native.knn_graph_constants()
    assert q == 64 and unroll >= 1
    assert (native.KNN_FEW_CANDIDATES, native.KNN_NAN_DISTANCE) == (1, 2)
    assert re.search(r"GNC_KNN_FEW_CANDIDATES\s*=\s*1\s*,\s*GNC_KNN_NAN_DISTANCE\s*=\s*2", header)


@pytest.mark.parametrize("k,dim,ld", [(0, 5, 5), (17, 5, 5), (8, 0, 5), (8, 17, 17), (8, 5, 4)])
def test_unsupported_shapes_are_refused_before_any_hip_call(k, dim, ld):
    """Null pointers everywhere: the answer comes from the shape alone."""
    lib = native.load_library()
    assert lib.gnc_knn_graph_f32(None, ld, dim, None, 1, 10, k, 0, None, 10 * max(k, 0), None, None, None) == GNC_ERR_UNSUPPORTED
    assert b"outside the supported set" in lib.gnc_last_error_string()
    assert lib.gnc_knn_graph_padded_f32(None, ld, dim, None, 4, 2, 16, k, 0, None, None, None, None) == GNC_ERR_UNSUPPORTED
    assert b"outside the supported set" in lib.gnc_last_error_string()


def test_python_side_errors_come_before_any_launch():
    feat = torch.zeros(10, 5)  # a CPU tensor: nothing below may get as far as the device
    with pytest.raises(ValueError, match="graph 1 has 3 nodes"):
        F.knn_graph(feat, 4, graph_ptr=[0, 7, 10])
    with pytest.raises(ValueError, match="graph 1 has 3 nodes"):
        F.knn_graph(feat, 3, graph_ptr=torch.tensor([0, 7, 10]))  # 3 nodes have 2 candidates each without self-loops
    with pytest.raises(ValueError, match="ascend"):
        F.knn_graph(feat, 2, graph_ptr=[0, 7, 9])
    for k in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            F.knn_graph(feat, k)
    with pytest.raises(NotImplementedError, match="float32"):
        F.knn_graph(feat.double(), 2)
    with pytest.raises(NotImplementedError, match="float32"):
        F.knn_graph(feat.half(), 2)
    with pytest.raises(NotImplementedError, match="17 feature columns"):
        F.knn_graph(torch.zeros(10, 17), 2)
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        F.knn_graph(torch.zeros(10), 2)


def test_unknown_edges_keyword():
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for method in I2G.METHODS:
        with pytest.raises(ValueError, match="Unknown edges"):
            I2G.graphs_from_images([img], method, edges="voxel")
    with pytest.raises(ValueError, match="knn_k"):
        I2G.graphs_from_images([img], "pixel", edges="knn", knn_k=17)
    assert I2G.graphs_from_images([], "pixel", edges="knn") == []


def test_reference_agrees_with_float64_on_tie_free_input():
    rng = np.random.default_rng(0)
    feat = rng.standard_normal((300, 5)).astype(np.float32)
    d64 = ((feat[:, None, :].astype(np.float64) - feat[None, :, :].astype(np.float64)) ** 2).sum(-1)
    np.fill_diagonal(d64, np.inf)
    want = np.argsort(d64, axis=1, kind="stable")[:, :8]
    gaps = np.diff(np.sort(d64, axis=1)[:, :9], axis=1)
    assert gaps.min() > 1e-5  # far above fp32 rounding of these sums: the float32 order is the float64 order
    nbr, fld, _ = R.knn_one_graph(feat, 8)
    assert np.array_equal(nbr, want)
    ei, bits = R.knn_graph(feat, 8)
    assert np.array_equal(ei[0].reshape(300, 8), want) and np.array_equal(ei[1], np.repeat(np.arange(300), 8))
    assert np.array_equal(bits.reshape(300, 8), fld)


def test_reference_ties_on_the_integer_grid():
    grid = R.integer_grid(9)
    assert grid.shape == (81, 2)
    assert R.rows_cut_inside_a_tie(grid, 3) == 49
    assert R.rows_cut_inside_a_tie(grid, 8) == 8
    nbr, fld, _ = R.knn_one_graph(grid, 3)
    # node 40 = (4, 4), the centre: four neighbours at distance 1, the three smallest ids win, in id order
    assert nbr[40].tolist() == [31, 39, 41] and fld[40].view(np.float32).tolist() == [1.0, 1.0, 1.0]
    # a corner: two at distance 1, then the diagonal at 2
    assert nbr[0].tolist() == [1, 9, 10] and fld[0].view(np.float32).tolist() == [1.0, 1.0, 2.0]


def test_reference_batches_loops_short_graphs_and_nan():
    rng = np.random.default_rng(1)
    feat = rng.standard_normal((12, 3)).astype(np.float32)
    ei, bits = R.knn_graph(feat, 4, graph_ptr=[0, 3, 12])
    first = ei[:, :12].reshape(2, 3, 4)
    assert (first[:, :, 2:] == -1).all() and (first[0, :, :2] >= 0).all() and (first[0, :, :2] < 3).all()
    assert (bits[:12].reshape(3, 4)[:, 2:] == 0x7F800000).all()
    alone, _ = R.knn_graph(feat[3:], 4)
    assert np.array_equal(ei[:, 12:], alone + 3)
    loop, lbits = R.knn_graph(feat, 2, loop=True)
    assert np.array_equal(loop[0, ::2], np.arange(12)) and (lbits[::2] == 0).all()
    feat[5, 1] = np.nan
    nbr, fld, _ = R.knn_one_graph(feat, 11)
    assert (nbr[np.arange(12) != 5, -1] == 5).all() and (fld[np.arange(12) != 5, -1] == 0xFFFFFFFF).all()
    assert nbr[5].tolist() == [u for u in range(12) if u != 5] and (fld[5] == 0xFFFFFFFF).all()
