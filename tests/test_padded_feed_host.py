"""Host-only: ``GNN.PaddedGraphFeed`` - the input buffers of every single-graph padded capture - on the CPU, against values written
out here.  5 nodes, ``node_capacity`` 8, ``edge_capacity`` 12: 2 dummies (rows 8 and 9), 10 rows."""
import pytest
import torch

EDGES = torch.tensor([[0, 1, 2, 3, 4], [1, 2, 3, 4, 0]])


class _AsIfOnDevice(torch.Tensor):
    """A CPU tensor that says it is a device tensor: the feed must not read it (that would synchronise) and flags instead."""
    is_cuda = True


def _sample(n, e=None, width=3):
    ei = EDGES[:, :0] if e == 0 else torch.arange(2 * (n if e is None else e)).reshape(2, -1) % n
    return torch.arange(1.0, n * width + 1).reshape(n, width), -torch.arange(1.0, n * 2 + 1).reshape(n, 2), ei


def _feed(node_capacity=8, n=5, **kw):
    from graphnet_classifier_amd.GNN import PaddedGraphFeed
    x, pos, _ = _sample(n)
    return PaddedGraphFeed(x, pos, EDGES, 12, node_capacity, device="cpu", **kw)


def test_buffers_after_construction():
    f = _feed()
    x, pos, _ = _sample(5)
    assert (f.rows, f.dummies, f.num_nodes, f.edge_capacity, f.node_capacity) == (10, 2, 5, 12, 8)
    assert f.x.shape == (10, 3) and f.pos.shape == (10, 2) and f.edge_index.shape == (2, 12) and f.edge_index.dtype == torch.int64
    assert torch.equal(f.x[:5], x) and torch.equal(f.pos[:5], pos) and not f.x[5:].any() and not f.pos[5:].any()
    assert torch.equal(f.edge_index[:, :5], EDGES)
    tail = [8 + k % 2 for k in range(5, 12)]
    assert f.edge_index[0, 5:].tolist() == tail and f.edge_index[1, 5:].tolist() == tail
    assert f.graph_ptr.tolist() == [0, 5] and int(f.valid_nodes) == 5 and not bool(f._range_flag)
    # without a node capacity the dummies stand behind the sample's own nodes; the flatten read-out may ask for more rows
    g = _feed(node_capacity=None)
    assert (g.rows, g.dummies) == (7, 2) and g.edge_index[0, 5:].tolist() == [5 + k % 2 for k in range(5, 12)]
    assert _feed(min_rows=16).rows == 16 and _feed(min_rows=4).rows == 10


def test_a_smaller_graph_after_a_larger_one():
    f = _feed()
    f(*_sample(7))
    assert f.num_nodes == 7 and int(f.valid_nodes) == 7 and bool(f.x[6].any()) and not f.x[7:].any()
    x, pos, ei = _sample(4)
    f(x, pos, ei)
    assert torch.equal(f.x[:4], x) and torch.equal(f.pos[:4], pos)
    assert not f.x[4:7].any() and not f.pos[4:7].any() and not f.x[7:].any()
    assert f.num_nodes == 4 and int(f.valid_nodes) == 4 and f.graph_ptr.tolist() == [0, 4]
    assert f.valid_nodes.data_ptr() == f.graph_ptr[1].data_ptr() and f.valid_nodes._base is f.graph_ptr  # the same storage
    assert torch.equal(f.edge_index[:, :4], ei) and f.edge_index[0, 4:].tolist() == [8 + k % 2 for k in range(4, 12)]


def test_no_edges_and_a_full_edge_list():
    f = _feed()
    x, pos, none = _sample(5, e=0)
    f(x, pos, none)
    dummies = [8 + k % 2 for k in range(12)]
    assert f.edge_index[0].tolist() == dummies and f.edge_index[1].tolist() == dummies
    x, pos, full = _sample(5, e=12)
    f(x, pos, full)
    assert full.shape == (2, 12) and torch.equal(f.edge_index, full)
    f(x, pos, EDGES)  # and the tail comes back behind a shorter list
    assert torch.equal(f.edge_index[:, :5], EDGES) and f.edge_index[1, 5:].tolist() == [8 + k % 2 for k in range(5, 12)]
    f.check(None)


@pytest.mark.parametrize("bad", [5, 8, -1])
def test_a_host_edge_list_outside_the_graph_raises_at_once(bad):
    """Row 5 is a slot of the capacity and row 8 a dummy: both inside the buffers, neither a node of this graph."""
    f = _feed()
    x, pos, ei = _sample(5)
    ei = ei.clone()
    ei[1, 2] = bad
    before = f.edge_index.clone()
    with pytest.raises(IndexError):
        f(x, pos, ei)
    assert torch.equal(f.edge_index, before) and not bool(f._range_flag)
    f.check(None)


def test_a_device_edge_list_outside_the_graph_raises_in_check_once():
    f = _feed()
    x, pos, ei = _sample(5)
    bad = ei.clone()
    bad[0, 1] = 5
    f(x, pos, bad.as_subclass(_AsIfOnDevice))  # no read, no raise
    assert bool(f._range_flag)
    f(x, pos, ei.as_subclass(_AsIfOnDevice))   # sticky: a clean edge list afterwards does not clear it
    assert bool(f._range_flag)
    with pytest.raises(IndexError):
        f.check(None)
    assert not bool(f._range_flag)
    f.check(None)
    f.check(torch.zeros(2, dtype=torch.int32))
    with pytest.raises(IndexError):            # the flags of the topology build inside the graph
        f.check(torch.tensor([0, 1], dtype=torch.int32))


def test_matches_refuses_what_does_not_fit():
    f = _feed()
    assert f.matches(_sample(5)) and f.matches(_sample(8, e=12)) and f.matches(_sample(1, e=0))
    assert not f.matches(_sample(9))                # too many nodes
    assert not f.matches(_sample(5, e=13))          # too many edges
    assert not f.matches(_sample(5, width=4))       # another feature width
    x, pos, ei = _sample(5)
    assert not f.matches((x, pos[:, :1], ei)) and not f.matches((x, pos, ei[0]))
    g = _feed(node_capacity=None)
    assert g.matches(_sample(5, e=12)) and not g.matches(_sample(4)) and not g.matches(_sample(6))  # one node count only
    for feed, sample in ((f, _sample(9)), (f, _sample(5, e=13)), (g, _sample(4))):
        with pytest.raises(ValueError, match="PaddedGraphFeed"):
            feed(*sample)
    with pytest.raises(ValueError, match="Mine"):   # the messages carry the owner's name
        _feed(who="Mine")(*_sample(9))
    from graphnet_classifier_amd.GNN import PaddedGraphFeed
    with pytest.raises(ValueError):
        PaddedGraphFeed(*_sample(9), 12, 8, device="cpu")
    with pytest.raises(ValueError):
        PaddedGraphFeed(*_sample(5, e=13), 12, 8, device="cpu")


def test_only_the_lenient_feed_keeps_what_a_call_leaves_out():
    x, pos, ei = _sample(5)
    f = _feed(node_capacity=None, keep_missing=True)  # CapturedForward's, edge_capacity form
    before = (f.pos.clone(), f.edge_index.clone())
    f(2 * x, None, None)
    assert torch.equal(f.x[:5], 2 * x) and torch.equal(f.pos, before[0]) and torch.equal(f.edge_index, before[1])
    f(x, pos, None)
    assert torch.equal(f.edge_index, before[1])
    for strict in (_feed(node_capacity=None), _feed(keep_missing=True)):  # CapturedTrainStep's; any feed under a node capacity
        with pytest.raises(ValueError, match="needs x, pos and edge_index"):
            strict(x, None, ei)
        with pytest.raises(ValueError, match="needs x, pos and edge_index"):
            strict(x, pos, None)


def test_every_capture_is_its_base_plus_a_feed():
    from graphnet_classifier_amd import GNN, train
    assert issubclass(train.CapturedRaggedBatchStep, train.CapturedTrainStep)
    assert issubclass(train.CapturedTensorStep, train.CapturedTrainStep)
    assert issubclass(GNN.CapturedRaggedBatchForward, GNN.CapturedForward)
    for cls in (train.CapturedRaggedBatchStep, train.CapturedTensorStep, GNN.CapturedRaggedBatchForward):
        assert "_record" not in vars(cls) and "check" not in vars(cls)  # one recording, one check: the base's
