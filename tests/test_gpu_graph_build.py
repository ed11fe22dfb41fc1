"""GPU parity of the device-side graph builders (csrc/graph_build.hip) against the golden vectors captured
from the reference's own pixel / patch builders (G6, G7) and against the oracle restatement of the
superpixel builder's post-SLIC part (unpinned: scikit-image is absent, see oracle/image_graph_oracle.py)."""
import numpy as np
import pytest
import torch

from oracle import image_graph_oracle as IO
from tests._util import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def I2G():
    from graphnet_classifier_amd import image_to_graph
    return image_to_graph


def test_grid_edges_match_reference_goldens(I2G):
    g = load_golden("g6_grid_edges.npz")
    for key, ref in g.items():
        _, hw, diag = key.split("_")
        h, w = (int(v) for v in hw.split("x"))
        ei = I2G.create_grid_edges_optimized(h, w, diag == "diag")
        assert ei.dtype == torch.int64 and np.array_equal(ei.cpu().numpy(), ref), key
    assert I2G.create_grid_edges_optimized(1, 1).shape == (2, 0)
    assert I2G.get_cached_edge_index(32, False) is I2G.get_cached_edge_index(32, False)  # lru_cache like optimized.py:42


@pytest.mark.parametrize("tag", ["muffin32", "chihuahua64"])
def test_pixel_and_patch_graphs_match_reference_goldens(I2G, tag):
    g = load_golden("g7_image_graphs.npz")
    img = g[f"{tag}/img"]
    for diag in (False, True):
        d = "diag" if diag else "nodiag"
        x, pos, ei = I2G.pixel_graph_from_array(img, diag)
        assert np.array_equal(x.cpu().numpy(), g[f"{tag}/pixel_{d}/x"])
        assert np.array_equal(pos.cpu().numpy(), g[f"{tag}/pixel_{d}/pos"])
        assert np.array_equal(ei.cpu().numpy(), g[f"{tag}/pixel_{d}/edge_index"])
    x, pos, ei = I2G.patch_graph_from_array(img, 8)
    assert np.array_equal(x.cpu().numpy(), g[f"{tag}/patch/x"])
    assert np.array_equal(pos.cpu().numpy(), g[f"{tag}/patch/pos"])
    assert np.array_equal(ei.cpu().numpy(), g[f"{tag}/patch/edge_index"])


def _voronoi_labels(rng, size, nseg, gaps=False):
    pts = rng.random((nseg, 2)) * size
    yy, xx = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    d = (yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2
    lab = d.argmin(-1).astype(np.int32)
    return lab * 3 + 1 if gaps else lab  # non-contiguous label values exercise the np.unique compaction


@pytest.mark.parametrize("size,nseg,gaps", [(8, 5, False), (32, 40, False), (32, 100, True), (64, 100, False)])
def test_superpixel_graph_from_labels_matches_oracle(I2G, size, nseg, gaps):
    rng = np.random.default_rng(size * 1000 + nseg)
    img = rng.integers(0, 256, size=(size, size, 3), dtype=np.uint8)
    seg = _voronoi_labels(rng, size, nseg, gaps)
    x, pos, ei = I2G.superpixel_graph_from_labels(img, seg)
    rx, rpos, rei = IO.superpixel_graph_from_labels(img, seg)
    assert x.shape == rx.shape and ei.shape == rei.shape
    assert np.array_equal(ei.cpu().numpy(), rei)               # same pairs, same order
    assert np.array_equal(pos.cpu().numpy(), rpos)             # integer sums / count: exact
    assert float(np.abs(x.cpu().numpy() - rx).max()) <= 6e-8   # float64 mean of k/255 vs exact integer sum / 255: <= 1 ulp


def _sides_beyond_two_passes():
    """(H, W) of the smallest near-square image with more than two passes of the builders' capped grid (8 workgroups of 256
    threads per CU, one pixel per thread and trip) and a ragged tail."""
    cap = 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    side = int((2 * cap) ** 0.5) + 1
    assert side * (side + 1) > 2 * cap
    return side, side + 1, cap


def test_pixel_graph_beyond_two_passes_of_the_capped_grid(I2G):
    h, w, cap = _sides_beyond_two_passes()
    img = np.random.default_rng(1).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    x, pos, ei = I2G.pixel_graph_from_array(img, True, use_cache=False)  # with diagonals: all four edge families
    rx, rpos, rei = IO.pixel_graph(img, True)
    assert rx.shape[0] > 2 * cap and rei.shape[1] > 2 * cap
    assert np.array_equal(x.cpu().numpy(), rx) and np.array_equal(pos.cpu().numpy(), rpos)
    assert ei.dtype == torch.int64 and np.array_equal(ei.cpu().numpy(), rei)


def test_patch_nodes_beyond_two_passes_of_the_capped_grid(I2G):
    """2 x 2 patches: one item per (patch, channel).  The reference formula of oracle.image_graph_oracle.patch_graph (float64
    mean of the uint8 patch, integer centres) vectorised over the patches."""
    h, w, cap = _sides_beyond_two_passes()
    img = np.random.default_rng(2).integers(0, 256, size=(2 * h, 2 * w + 1, 3), dtype=np.uint8)  # the last column joins no patch
    assert h * w * 3 > 2 * cap
    x, pos, ei = I2G.patch_graph_from_array(img, 2)
    want = img[:, :2 * w].reshape(h, 2, w, 2, 3).astype(np.float64).mean(axis=(1, 3)).reshape(h * w, 3).astype(np.float32)
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert np.array_equal(x.cpu().numpy(), want)
    assert np.array_equal(pos.cpu().numpy(), np.stack([2 * ii.ravel() + 1, 2 * jj.ravel() + 1], axis=1).astype(np.float32))
    small = IO.patch_graph(img[:12, :14], 2)  # ... which is the oracle's loop, patch by patch
    assert np.array_equal(want.reshape(h, w, 3)[:6, :7].reshape(-1, 3), small[0])


def test_superpixel_graph_from_labels_beyond_two_passes_of_the_capped_grid(I2G):
    """Rectangular segments with seeded cut positions (label values with gaps): the per-pixel launches of the region-adjacency
    build make a third trip; the oracle's dilation loop stays fast at 30 segments."""
    h, w, cap = _sides_beyond_two_passes()
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    rows = np.searchsorted(np.sort(rng.choice(np.arange(1, h), size=4, replace=False)), np.arange(h), side="right")
    cols = np.searchsorted(np.sort(rng.choice(np.arange(1, w), size=5, replace=False)), np.arange(w), side="right")
    seg = ((rows[:, None] * 6 + cols[None, :]) * 3 + 1).astype(np.int32)
    assert seg.size > 2 * cap and np.unique(seg).size == 30
    x, pos, ei = I2G.superpixel_graph_from_labels(img, seg)
    rx, rpos, rei = IO.superpixel_graph_from_labels(img, seg)
    assert x.shape == rx.shape and ei.shape == rei.shape
    assert np.array_equal(ei.cpu().numpy(), rei)
    assert np.array_equal(pos.cpu().numpy(), rpos)
    assert float(np.abs(x.cpu().numpy() - rx).max()) <= 6e-8


def _single_pixel_segment_graph(img):
    """The oracle's answer when every pixel is its own segment, in closed form: x = img / 255, pos = (row, col), and the
    4-neighbour pairs (p, p + 1), (p, p + W) in lexicographic order, each as [i, j], [j, i]."""
    h, w, _ = img.shape
    p = np.arange(h * w).reshape(h, w)
    lo = np.concatenate([p[:, :-1].ravel(), p[:-1].ravel()])
    hi = np.concatenate([p[:, 1:].ravel(), p[1:].ravel()])
    order = np.lexsort((hi, lo))
    lo, hi = lo[order], hi[order]
    ei = np.stack([np.stack([lo, hi], axis=1).ravel(), np.stack([hi, lo], axis=1).ravel()]).astype(np.int64)
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return ((img.reshape(-1, 3).astype(np.float64) / 255.0).astype(np.float32),
            np.stack([rr.ravel(), cc.ravel()], axis=1).astype(np.float32), ei)


def test_superpixel_graph_of_single_pixel_segments_beyond_two_passes(I2G):
    """The per-SEGMENT and per-PAIR launches (node features, edge list) make their later trips only with more segments than
    threads: every pixel its own label."""
    rng = np.random.default_rng(4)
    small = rng.integers(0, 256, size=(6, 7, 3), dtype=np.uint8)
    for got, want in zip(_single_pixel_segment_graph(small), IO.superpixel_graph_from_labels(small, np.arange(42).reshape(6, 7))):
        assert np.array_equal(got, want)  # the closed form is the oracle's loop
    h, w, cap = _sides_beyond_two_passes()
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    x, pos, ei = I2G.superpixel_graph_from_labels(img, np.arange(h * w, dtype=np.int32).reshape(h, w))
    rx, rpos, rei = _single_pixel_segment_graph(img)
    assert rx.shape[0] > 2 * cap and rei.shape[1] // 2 > 2 * cap
    assert np.array_equal(ei.cpu().numpy(), rei) and np.array_equal(pos.cpu().numpy(), rpos) and np.array_equal(x.cpu().numpy(), rx)


def test_superpixel_graph_rejects_bad_labels(I2G):
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    seg = np.zeros((4, 4), dtype=np.int32)
    seg[1, 1] = 99
    with pytest.raises(ValueError):
        I2G.superpixel_graph_from_labels(img, seg)


def test_builders_feed_the_model(I2G):
    """End to end on the device: shipped-image pixel graph -> CombinedModel logits, no host round trip."""
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    g = load_golden("g7_image_graphs.npz")
    x, pos, ei = I2G.pixel_graph_from_array(g["muffin32/img"])
    torch.manual_seed(0)
    m = CombinedModel(GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=2, out_dim_node=32, out_dim_edge=32,
                               hidden_dim_node=32, hidden_dim_edge=32, hidden_dim_decoder=32, hidden_dim_processor_node=32,
                               hidden_dim_processor_edge=32), num_nodes=1024, classes=2)
    with torch.no_grad():
        logits = m((x, pos, ei))
    assert logits.is_cuda and logits.shape == (2,) and bool(torch.isfinite(logits).all())
