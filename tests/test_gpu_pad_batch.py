"""GPU: the feed launch of a captured ragged-batch step (``native.pad_graph_batch`` -> ``gnc_pad_graph_batch``).  Every buffer it
writes - x, pos, the edge list with its dummy tail, graph_ptr, labels - is compared bit for bit with the rule stated in NumPy
below; rows it must not write (the dummies) are checked for the sentinel they held.  Graphs: 9, 12 or 16 nodes each."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((3, 3), (3, 4), (4, 4))
SENTINEL = -7.0


def _batch(G, seed, fx=3):
    from graphnet_classifier_amd import synthetic
    b = synthetic.superpixel_like_graphs(G, seed, shapes=SHAPES)
    if fx != 3:
        b.x = torch.from_numpy(np.random.default_rng(seed).random((b.num_nodes, fx), dtype=np.float32))
    return b


def _expected(x, pos, ei, graph_ptr, labels, M, C):
    """The rule: node slots [0, M) hold the batch then zeros, D = max(1, ceil(C / 8)) dummies behind them are left alone, edge
    slots behind the batch's E edges are self-loops of dummy M + k % D."""
    D = max(1, -(-C // 8))
    N, E = x.shape[0], ei.shape[1]
    xb = np.full((M + D, x.shape[1]), SENTINEL, dtype=np.float32)
    pb = np.full((M + D, pos.shape[1]), SENTINEL, dtype=np.float32)
    xb[:M], pb[:M] = 0.0, 0.0
    xb[:N], pb[:N] = x, pos
    eb = np.tile(M + np.arange(C, dtype=np.int64) % D, (2, 1))
    eb[:, :E] = ei
    return xb, pb, eb, np.asarray(graph_ptr, dtype=np.int64), None if labels is None else np.asarray(labels, dtype=np.int64)


def _leaves_its_graph(ei, graph_ptr, edge_ptr):
    g = np.searchsorted(np.asarray(edge_ptr)[1:], np.arange(ei.shape[1]), side="right")
    lo, hi = np.asarray(graph_ptr)[g], np.asarray(graph_ptr)[g + 1]
    return bool(((ei < lo) | (ei >= hi)).any())


class _Buffers:
    def __init__(self, G, M, C, fx=3, fp=2, labels=True):
        from graphnet_classifier_amd import native
        self.M, self.C = M, C
        self.rows, self.D = native.ragged_batch_layout(M, C)
        self.x = torch.full((self.rows, fx), SENTINEL, device=DEV)
        self.pos = torch.full((self.rows, fp), SENTINEL, device=DEV)
        self.ei = torch.full((2, C), -1, dtype=torch.int64, device=DEV)
        self.gp = torch.full((G + 1,), -1, dtype=torch.int64, device=DEV)
        self.labels = torch.full((G,), -1, dtype=torch.int64, device=DEV) if labels else None
        self.flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def feed(self, x, pos, ei, graph_ptr, edge_ptr, labels=None):
        from graphnet_classifier_amd import native
        native.pad_graph_batch(x, pos, ei, graph_ptr, edge_ptr, labels, self.M, self.C, self.x, self.pos, self.ei, self.gp,
                               self.labels if labels is not None else None, self.flag)

    def check(self, x, pos, ei, graph_ptr, labels=None):
        want = _expected(x.cpu().numpy(), pos.cpu().numpy(), ei.cpu().numpy(), graph_ptr, labels, self.M, self.C)
        got = (self.x, self.pos, self.ei, self.gp, self.labels if labels is not None else None)
        for name, w, g in zip(("x", "pos", "edge_index", "graph_ptr", "labels"), want, got):
            if w is not None:
                assert np.array_equal(g.cpu().numpy(), w), name


def _feed_and_check(buf, b, labels=None):
    d = b.to(DEV)
    buf.feed(d.x, d.pos, d.edge_index, b.graph_ptr, b.edge_ptr, labels)
    buf.check(b.x, b.pos, b.edge_index, b.graph_ptr.tolist(), labels)


def test_three_graphs_then_a_smaller_batch_into_the_same_buffers():
    big, small = _batch(3, 13), _batch(3, 11)  # 48 nodes / 198 edges, then 34 / 130
    assert small.num_nodes < big.num_nodes and small.num_edges < big.num_edges
    buf = _Buffers(3, 64, 256)
    lab = [1, 0, 1]
    _feed_and_check(buf, big, lab)
    # rows [N2, N1) are zero again and the dummy tail is restored behind the shorter edge list
    _feed_and_check(buf, small, torch.tensor([0, 0, 1]))
    assert int(buf.flag.item()) == 0


def test_no_slack_and_no_tail():
    b = _batch(3, 21)
    buf = _Buffers(3, b.num_nodes, b.num_edges)
    _feed_and_check(buf, b, [0, 1, 0])
    assert int(buf.flag.item()) == 0


@pytest.mark.parametrize("G", [1, 64])
def test_one_graph_and_the_most_graphs(G):
    b = _batch(G, 30 + G)
    buf = _Buffers(G, (b.num_nodes + 31) // 32 * 32 + 5, b.num_edges + 37)  # an odd edge capacity: row 1 of ei_buf is 8-B aligned only
    _feed_and_check(buf, b, list(range(G)))
    assert int(buf.flag.item()) == 0


def test_a_graph_without_edges():
    from graphnet_classifier_amd import synthetic
    b = _batch(3, 41)
    e0, e1 = int(b.edge_ptr[1]), int(b.edge_ptr[2])
    keep = torch.cat([torch.arange(e0), torch.arange(e1, b.num_edges)])
    edge_ptr = torch.tensor([0, e0, e0, b.num_edges - (e1 - e0)])
    b = synthetic.GraphBatch(b.x, b.pos, b.edge_index[:, keep].contiguous(), b.graph_ptr, edge_ptr)
    buf = _Buffers(3, 64, 256)
    _feed_and_check(buf, b, [1, 1, 0])
    assert int(buf.flag.item()) == 0
    # the same with NO edge at all in the batch
    none = synthetic.GraphBatch(b.x, b.pos, b.edge_index[:, :0].contiguous(), b.graph_ptr, torch.zeros(4, dtype=torch.int64))
    _feed_and_check(buf, none, [1, 1, 0])
    assert int(buf.flag.item()) == 0


def test_five_node_features():
    b = _batch(3, 51, fx=5)
    buf = _Buffers(3, 64, 256, fx=5)
    _feed_and_check(buf, b, [0, 1, 1])


def test_sources_that_are_views_at_four_byte_alignment():
    """``[1:]`` views of larger tensors: x / pos start 12 / 8 bytes into their allocation, the edge rows 8 bytes (and have a row
    stride of E + 1)."""
    b = _batch(3, 61)
    x = torch.cat([torch.zeros(1, 3), b.x]).to(DEV)[1:]
    pos = torch.cat([torch.zeros(1, 2), b.pos]).to(DEV)[1:]
    ei = torch.cat([torch.zeros(2, 1, dtype=torch.int64), b.edge_index], dim=1).to(DEV)[:, 1:]
    assert x.data_ptr() % 16 == 12 and pos.data_ptr() % 16 == 8 and ei.data_ptr() % 16 == 8 and ei.stride(0) == b.num_edges + 1
    buf = _Buffers(3, 64, 256)
    buf.feed(x, pos, ei, b.graph_ptr, b.edge_ptr, [1, 0, 0])
    buf.check(b.x, b.pos, b.edge_index, b.graph_ptr.tolist(), [1, 0, 0])
    assert int(buf.flag.item()) == 0


def test_without_labels_the_label_buffer_is_not_written():
    b = _batch(3, 71)
    buf = _Buffers(3, 64, 256)
    _feed_and_check(buf, b, None)
    assert buf.labels.tolist() == [-1, -1, -1]


def _bad_batches():
    b = _batch(3, 81)
    gp = b.graph_ptr.tolist()
    rows = 64 + 32
    k = int(b.edge_ptr[1]) + 1  # an edge of graph 1
    cases = {"into_another_graph": gp[2], "below_its_graph": gp[1] - 1, "slack_row": b.num_nodes + 1, "dummy_row": 64 + 3,
             "negative": -1, "at_rows": rows, "far_outside": 1 << 40}
    for name, value in cases.items():
        for end in (0, 1):
            ei = b.edge_index.clone()
            ei[end, k] = value
            yield f"{name}-end{end}", b, ei


@pytest.mark.parametrize("name", [n for n, _, _ in _bad_batches()])
def test_an_edge_that_leaves_its_graph_sets_the_sticky_flag(name):
    b, ei = next((bb, e) for n, bb, e in _bad_batches() if n == name)
    assert _leaves_its_graph(ei.numpy(), b.graph_ptr.tolist(), b.edge_ptr.tolist())
    buf = _Buffers(3, 64, 256)
    d = b.to(DEV)
    buf.feed(d.x, d.pos, ei.to(DEV), b.graph_ptr, b.edge_ptr, [0, 1, 0])
    buf.check(b.x, b.pos, ei, b.graph_ptr.tolist(), [0, 1, 0])  # the ids are copied as given
    assert int(buf.flag.item()) == 1
    # sticky: a clean batch afterwards leaves it set; only the host clears it
    clean = _batch(3, 82)
    assert not _leaves_its_graph(clean.edge_index.numpy(), clean.graph_ptr.tolist(), clean.edge_ptr.tolist())
    _feed_and_check(buf, clean, [1, 1, 1])
    assert int(buf.flag.item()) == 1
    buf.flag.zero_()
    _feed_and_check(buf, clean, [1, 1, 1])
    assert int(buf.flag.item()) == 0


def test_a_feed_of_more_than_two_passes_of_the_capped_grid():
    """The launch is capped at 4 workgroups per CU (1024 x CUs threads, one 16-byte chunk each per trip): 64 graphs large enough
    that x, pos AND the edge rows each reach into a later trip of the grid-stride loop, with an odd edge capacity and slack."""
    from graphnet_classifier_amd import synthetic
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    side = int((5 * cus) ** 0.5) + 2
    b = synthetic.superpixel_like_graphs(64, 101, shapes=((side, side), (side, side + 1)))
    M, C = b.num_nodes + 37, b.num_edges + 1027
    chunks_x, chunks_pos, chunks_row = -(-M * 3 // 4), -(-M * 2 // 4), -(-C // 2)
    total = chunks_x + chunks_pos + 2 * chunks_row + 2 * 64 + 1
    assert total > 2 * 1024 * cus, "the capped grid must make a third trip"
    assert chunks_x + chunks_pos < 1024 * cus < chunks_x + chunks_pos + chunks_row  # the first pass ends inside edge row 0
    buf = _Buffers(64, M, C)
    _feed_and_check(buf, b, list(range(64)))
    assert int(buf.flag.item()) == 0


def test_sixty_five_graphs_raise_on_the_host_and_nothing_is_launched():
    from graphnet_classifier_amd import native
    b = _batch(65, 91)
    buf = _Buffers(65, 1088, 4096)
    d = b.to(DEV)
    timers = native.KernelTimers()
    native.set_kernel_timers(timers)
    try:
        with pytest.raises(ValueError):
            buf.feed(d.x, d.pos, d.edge_index, b.graph_ptr, b.edge_ptr, list(range(65)))
        with pytest.raises(ValueError):  # above a capacity: the same
            small = _Buffers(3, 16, 256)
            three = _batch(3, 92).to(DEV)
            small.feed(three.x, three.pos, three.edge_index, three.graph_ptr, three.edge_ptr, [0, 0, 0])
    finally:
        native.set_kernel_timers(None)
    assert timers.num_launches() == 0
    assert bool((buf.x == SENTINEL).all()) and bool((buf.ei == -1).all()) and bool((buf.gp == -1).all())
    assert int(buf.flag.item()) == 0
