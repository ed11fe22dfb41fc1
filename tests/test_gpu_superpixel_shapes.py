"""GPU: the device SLIC (csrc/superpixel.hip) against the sequential NumPy oracle (oracle/slic_oracle.py) at the shapes of
tests/superpixel_shape_cases.py: partly filled 16 x 16 tiles, ragged centre boxes, thin and one-pixel images, unit steps,
1089 centres, boxes wider than a wave.  Labels are integers: every comparison is bit for bit.

The fixtures of tests/test_gpu_superpixel.py all have sides that are multiples of the tile; the oracle is pinned to those
same fixtures by tests/test_slic_oracle_host.py, which also holds the case table to its conditions."""
import numpy as np
import pytest
import torch

from oracle import image_graph_oracle as IO
from tests import superpixel_shape_cases as S

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in S.CASES]


@pytest.fixture(scope="module")
def I2G():
    from graphnet_classifier_amd import image_to_graph
    return image_to_graph


def _conn(kw):
    return kw.get("enforce_connectivity", True)


def _compare(I2G, img, kw, ref, info):
    labels, counts = I2G.slic(img, **kw, return_counts=True)
    got = labels.cpu().numpy()
    assert labels.dtype == torch.int32 and labels.is_cuda and got.shape == ref.shape and counts.shape == (1,)
    mism = int((got != ref).sum())
    assert mism == 0, f"{mism} of {ref.size} pixels differ from the sequential oracle"
    if _conn(kw):
        assert int(counts[0]) == info["n_labels"]
    else:
        assert int(counts[0]) == info["K"]
        assert not (got == kw.get("start_label", 0) - 1).any()  # every pixel was inside some centre's window


@pytest.mark.parametrize("name", NAMES)
def test_labels_equal_the_sequential_oracle(I2G, name):
    _, img, kw = S.BY_NAME[name]
    ref, info = S.oracle(name)
    _compare(I2G, img, kw, ref, info)


@pytest.mark.parametrize("name", [n for n in NAMES if not _conn(S.BY_NAME[n][2])])
def test_start_label_one_is_plus_one_without_connectivity(I2G, name):
    _, img, kw = S.BY_NAME[name]
    zero, c0 = I2G.slic(img, **dict(kw, start_label=0), return_counts=True)
    one, c1 = I2G.slic(img, **dict(kw, start_label=1), return_counts=True)
    assert torch.equal(one, zero + 1) and torch.equal(c0, c1)
    assert int(zero.min()) >= 0


@pytest.mark.parametrize("name", S.START_LABEL_CASES)
def test_start_label_one_with_connectivity_equals_the_oracle(I2G, name):
    # not "start_label = 0 plus one": a small component without a labelled neighbour is set to 0 under either start label
    _, img, kw = S.BY_NAME[name]
    kw = dict(kw, start_label=1)
    ref, info = S.oracle_at(name, **kw)
    _compare(I2G, img, kw, ref, info)


@pytest.mark.parametrize("connectivity", [True, False], ids=["conn1", "conn0"])
@pytest.mark.parametrize("shape", list(S.BATCH_CASES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_equals_per_image_at_partial_tiles(I2G, shape, connectivity):
    names = S.BATCH_CASES[shape]
    kw = dict(n_segments=100, enforce_connectivity=connectivity)
    batch = np.stack([S.BY_NAME[n][1] for n in names])
    labels, counts = I2G.slic(batch, **kw, return_counts=True)
    assert labels.shape == (5,) + shape and counts.shape == (5,)
    for i in range(5):
        li, ci = I2G.slic(batch[i], **kw, return_counts=True)
        assert torch.equal(li, labels[i]) and int(ci[0]) == int(counts[i])
    ref, info = S.oracle_at(names[S.BATCH_ORACLE_IMAGE], **kw)
    got = labels[S.BATCH_ORACLE_IMAGE].cpu().numpy()
    mism = int((got != ref).sum())
    assert mism == 0, f"{mism} of {ref.size} pixels of image {S.BATCH_ORACLE_IMAGE} differ from the sequential oracle"
    assert int(counts[S.BATCH_ORACLE_IMAGE]) == info["n_labels"]


@pytest.mark.parametrize("per_pixel_centres", [False, True], ids=["n100", "one_centre_per_pixel"])
def test_batch_beyond_two_passes_of_the_capped_grid_equals_per_image(I2G, per_pixel_centres):
    """The per-pixel launches (Lab conversion, plain labels) and the per-centre seeding run at most 8 workgroups of 256 threads
    per CU.  Five images that each fit in ONE pass, as a batch of more than two passes: the batch must give each image's own
    labels.  With one centre per pixel (unit steps) the seeding of the batch's centres takes its later trips too."""
    cap = 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    side = int((2 * cap / 5) ** 0.5) + 2
    assert side * side <= cap and 5 * side * side > 2 * cap
    rng = np.random.default_rng(side)
    batch = rng.integers(0, 256, size=(5, side, side, 3), dtype=np.uint8)
    kw = dict(n_segments=side * side if per_pixel_centres else 100, enforce_connectivity=False, max_iter=2)
    alone = [I2G.slic(batch[i], **kw, return_counts=True) for i in range(5)]
    centres = int(alone[0][1][0])  # without the connectivity pass: K, the number of centres
    assert not per_pixel_centres or (centres <= cap and 5 * centres > 2 * cap)
    labels, counts = I2G.slic(batch, **kw, return_counts=True)
    for i in range(5):
        assert torch.equal(labels[i], alone[i][0]) and int(counts[i]) == int(alone[i][1][0]) == centres
    assert int(labels.min()) >= 0 and int(labels.max()) < centres


def test_repeated_calls_give_the_same_labels(I2G):
    """the box atomics of slic_assign and a workspace that an earlier call of another shape has used"""
    first = {}
    for name in ("100x100-n1000-noise-conn0-emptied", "33x48-n100-blobs", "100x100-n1000-noise-conn0-emptied",
                 "100x100-n100-blobs", "33x48-n100-blobs", "100x100-n100-blobs"):
        _, img, kw = S.BY_NAME[name]
        labels, counts = I2G.slic(img, **kw, return_counts=True)
        if name in first:
            assert torch.equal(labels, first[name][0]) and torch.equal(counts, first[name][1])
        else:
            first[name] = (labels, counts)


@pytest.fixture(scope="module")
def oracle_graphs():
    """the reference's graph construction (oracle restatement, pinned to the fixture graphs) on the ORACLE's labels"""
    out = {}
    for name in S.GRAPH_CASES:
        labels, _ = S.oracle(name)
        out[name] = IO.superpixel_graph_from_labels(S.BY_NAME[name][1], labels)
    return out


def _assert_graph(graph, ref):
    x, pos, ei = graph
    rx, rpos, rei = ref
    assert x.shape == rx.shape and ei.dtype == torch.int64 and tuple(ei.shape) == rei.shape
    assert np.array_equal(ei.cpu().numpy(), rei)
    assert np.array_equal(pos.cpu().numpy(), rpos)
    assert float(np.abs(x.cpu().numpy() - rx).max()) <= 6e-8


@pytest.mark.parametrize("name", S.GRAPH_CASES)
def test_graph_from_array_equals_the_graph_of_the_oracles_labels(I2G, oracle_graphs, name):
    _, img, kw = S.BY_NAME[name]
    n, c = kw["n_segments"], kw.get("compactness", 10.0)
    _assert_graph(I2G.superpixel_graph_from_array(img, n, c), oracle_graphs[name])


@pytest.mark.parametrize("name", S.GRAPH_CASES)
def test_batched_graphs_equal_the_per_image_graphs(I2G, oracle_graphs, name):
    _, img, kw = S.BY_NAME[name]
    n, c = kw["n_segments"], kw.get("compactness", 10.0)
    imgs = np.stack([img, img[::-1, ::-1], np.roll(img, 5, axis=1)])
    nodes, edges = I2G.superpixel_capacities(n)
    batch = I2G.superpixel_graphs_batched(imgs, n_segments=n, compactness=c, node_capacity=nodes, edge_capacity=edges)
    for b in range(3):
        x, pos, ei = I2G.superpixel_graph_from_array(imgs[b], n, c)
        s, e, bad, overflow = batch.counts[b].tolist()
        assert (s, e, bad) == (x.size(0), ei.size(1), 0)
        assert overflow == int(s > nodes or e > edges)
        if not overflow:
            assert torch.equal(batch.x[b, :s], x) and torch.equal(batch.pos[b, :s], pos)
            assert torch.equal(batch.edge_index[b, :, :e], ei)
    s, e, _, overflow = batch.counts[0].tolist()
    assert overflow == 0  # the case's own graph fits the capacities (tests/test_slic_oracle_host.py)
    _assert_graph((batch.x[0, :s], batch.pos[0, :s], batch.edge_index[0, :, :e]), oracle_graphs[name])
