"""GPU: the batched region-adjacency build (csrc/rag_batched.hip) against the reference's superpixel graphs and the
per-image build ``gnc_rag_build`` (tests/golden/g10_superpixel*.npz): whole batches bit for bit, padding, labels with
gaps, degenerate images, bad labels, overflow of either capacity with guard rows, and the loader on top of it."""
import collections

import numpy as np
import pytest
import torch

from tests.test_superpixel_golden import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def I2G():
    from graphnet_classifier_amd import image_to_graph
    return image_to_graph


def _by_size(cases):
    groups = collections.OrderedDict()
    for c in cases:
        groups.setdefault(c[1].shape[:2], []).append(c)
    return groups


def _build(I2G, cases, node_capacity=512, edge_capacity=2048):
    imgs = np.stack([c[1] for c in cases])
    labels = np.stack([c[2] for c in cases])
    return I2G.superpixel_graphs_batched(imgs, labels, node_capacity=node_capacity, edge_capacity=edge_capacity)


def _graph(batch, b):
    s, e, _, _ = batch.counts[b].tolist()
    return batch.x[b, :s], batch.pos[b, :s], batch.edge_index[b, :, :e]


def _assert_padding(batch, b):
    s, e, _, overflow = batch.counts[b].tolist()
    if overflow:
        s = e = 0
    assert not batch.x[b, s:].any() and not batch.pos[b, s:].any()
    assert bool((batch.edge_index[b, :, e:] == -1).all())


def test_reference_graphs_in_batches(I2G):
    seen = 0
    for shape, cases in _by_size([c for c in CASES if c[4] is not None]).items():
        batch = _build(I2G, cases)
        assert batch.x.is_cuda and batch.edge_index.dtype == torch.int64 and batch.counts.dtype == torch.int32
        for b, (_, _, _, _, (rx, rpos, rei)) in enumerate(cases):
            x, pos, ei = _graph(batch, b)
            assert batch.counts[b].tolist() == [rx.shape[0], rei.shape[1], 0, 0]
            assert np.array_equal(ei.cpu().numpy(), rei)
            assert float(np.abs(x.cpu().numpy() - rx).max()) <= 1e-6
            assert float(np.abs(pos.cpu().numpy() - rpos).max()) <= 1e-6
            seen += 1
    assert seen == 26


def test_every_case_equals_the_per_image_build(I2G):
    groups = _by_size(CASES)
    assert len(groups[(128, 128)]) == 18 and sum(len(g) for g in groups.values()) == 44
    for shape, cases in groups.items():
        batch = _build(I2G, cases)  # one call per image size: the 18 cases of 128 x 128 at 512 nodes / 2048 edges
        for b, (_, img, labels, _, _) in enumerate(cases):
            x, pos, ei = I2G.superpixel_graph_from_labels(img, labels)
            bx, bpos, bei = _graph(batch, b)
            assert batch.counts[b].tolist() == [x.size(0), ei.size(1), 0, 0]
            assert torch.equal(bx, x) and torch.equal(bpos, pos) and torch.equal(bei, ei)
            _assert_padding(batch, b)


def test_labels_with_gaps_and_degenerate_images(I2G):
    cases = [c for c in CASES if c[1].shape[:2] == (64, 64)][:4]
    dense = _build(I2G, cases)
    gaps = I2G.superpixel_graphs_batched(np.stack([c[1] for c in cases]), np.stack([3 * c[2] + 5 for c in cases]),
                                         node_capacity=512, edge_capacity=2048)
    for t, u in zip(dense, gaps):
        assert torch.equal(t, u)
    img = np.stack([c[1] for c in cases])
    one = I2G.superpixel_graphs_batched(img, np.full((4, 64, 64), 7, np.int32), node_capacity=16, edge_capacity=16)
    for b in range(4):
        assert one.counts[b].tolist() == [1, 0, 0, 0]
        mean = (img[b].reshape(-1, 3).astype(np.float64).sum(0) / 255.0 / 4096).astype(np.float32)
        assert np.array_equal(one.x[b, 0].cpu().numpy(), mean) and one.pos[b, 0].tolist() == [31.5, 31.5]
        _assert_padding(one, b)
    pixel = I2G.superpixel_graphs_batched(img[:2, :1, :1], np.zeros((2, 1, 1), np.int32), node_capacity=1, edge_capacity=1)
    assert pixel.counts.tolist() == [[1, 0, 0, 0]] * 2 and pixel.pos.flatten().tolist() == [0.0] * 4
    assert bool((pixel.edge_index == -1).all())


def test_bad_labels_flag_their_own_image_only(I2G):
    cases = [c for c in CASES if c[1].shape[:2] == (64, 64)][:4]
    labels = np.stack([c[2] for c in cases]).copy()
    labels[1, 10, 10] = 64 * 64
    labels[3, 0, 0] = -1
    imgs = np.stack([c[1] for c in cases])
    batch = I2G.superpixel_graphs_batched(imgs, labels, node_capacity=512, edge_capacity=2048)
    assert batch.counts[:, 2].tolist() == [0, 1, 0, 1]
    for b in (0, 2):
        x, pos, ei = I2G.superpixel_graph_from_labels(cases[b][1], cases[b][2])
        bx, bpos, bei = _graph(batch, b)
        assert torch.equal(bx, x) and torch.equal(bpos, pos) and torch.equal(bei, ei)
    with pytest.raises(ValueError, match="outside"):
        I2G._superpixel_graphs_from_device_batch(torch.from_numpy(imgs).cuda(), torch.from_numpy(labels).cuda(), 512, 2048)


def _guarded_build(I2G, cases, node_capacity, edge_capacity):
    """The kernel on buffers with one guard row behind each output: (batch, guards untouched)."""
    from graphnet_classifier_amd import native
    lib = native.load_library()
    dev = torch.device("cuda")
    imgs = torch.from_numpy(np.stack([c[1] for c in cases])).to(dev)
    labels = torch.from_numpy(np.stack([c[2] for c in cases])).to(dev)
    B, H, W, _ = imgs.shape
    x = torch.full((B + 1, node_capacity, 3), 7.0, device=dev)
    pos = torch.full((B + 1, node_capacity, 2), 7.0, device=dev)
    ei = torch.full((B + 1, 2, edge_capacity), 7, dtype=torch.int64, device=dev)
    counts = torch.full((B + 1, 4), 7, dtype=torch.int32, device=dev)
    nbytes = lib.gnc_rag_batched_workspace_bytes(B, H, W, node_capacity, edge_capacity)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    native._check(lib.gnc_rag_build_batched(labels.data_ptr(), imgs.data_ptr(), B, H, W, node_capacity, edge_capacity,
                                            x.data_ptr(), pos.data_ptr(), ei.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                            nbytes, torch.cuda.current_stream().cuda_stream), "gnc_rag_build_batched")
    torch.cuda.synchronize()
    intact = bool((x[B] == 7).all() and (pos[B] == 7).all() and (ei[B] == 7).all() and (counts[B] == 7).all())
    return I2G.SuperpixelGraphBatch(x[:B], pos[:B], ei[:B], counts[:B]), intact


@pytest.mark.parametrize("node_capacity,edge_capacity", [(100, 2048), (512, 500)], ids=["nodes100", "edges500"])
def test_overflow_flags_true_sizes_and_guards(I2G, node_capacity, edge_capacity):
    cases = [c for c in CASES if c[1].shape[:2] == (64, 64) and c[3] == (100, 10.0, 10, True)]
    assert len(cases) == 8
    per_image = [I2G.superpixel_graph_from_labels(c[1], c[2]) for c in cases]
    exceeds = [x.size(0) > node_capacity or ei.size(1) > edge_capacity for x, _, ei in per_image]
    assert any(exceeds) and not all(exceeds)
    if node_capacity == 100:
        assert sum(exceeds) == 5
    batch, intact = _guarded_build(I2G, cases, node_capacity, edge_capacity)
    assert intact, "the kernel wrote behind its output buffers"
    for b, (x, pos, ei) in enumerate(per_image):
        assert batch.counts[b].tolist() == [x.size(0), ei.size(1), 0, int(exceeds[b])]  # true sizes either way
        if not exceeds[b]:
            bx, bpos, bei = _graph(batch, b)
            assert torch.equal(bx, x) and torch.equal(bpos, pos) and torch.equal(bei, ei)
        _assert_padding(batch, b)


def test_loader_equals_per_image_builders(I2G):
    imgs = [c[1] for c in CASES if c[1].shape == (64, 64, 3)]
    batch = np.stack([imgs[i % len(imgs)] for i in range(24)])
    batch[8:] = np.roll(batch[8:], 3, axis=2)
    batch[16:] = batch[16:, ::-1]
    want = [I2G.superpixel_graph_from_array(im) for im in batch]
    sizes = {int(x.size(0)) for x, _, _ in want}
    assert len(sizes) >= 3
    low = sorted(int(x.size(0)) for x, _, _ in want)[12]  # about half of the images take the per-image path
    for kw in ({}, {"node_capacity": low}, {"edge_capacity": 450}, {"node_capacity": 513}):
        got = I2G.graphs_from_images(list(batch), method="superpixel", resize_value=64, **kw)
        assert len(got) == 24
        for (x, pos, ei), (wx, wpos, wei) in zip(got, want):
            assert torch.equal(x, wx) and torch.equal(pos, wpos) and torch.equal(ei, wei)
            assert ei.dtype == torch.int64 and x.is_cuda
