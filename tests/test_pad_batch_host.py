"""Host-only checks behind the captured ragged-batch step: the feed launch's C ABI (``gnc_pad_graph_batch`` and its ``supported``
query, declared, exported, answered without a GPU), the buffer layout ``ragged_batch_layout`` and the capacity rule."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gnc_pad_graph_batch", "gnc_pad_graph_batch_supported")


def test_library_exports_the_feed_launch_and_the_header_declares_it():
    from graphnet_classifier_amd import native
    lib = native.load_library()
    with open(os.path.join(ROOT, "include", "gnc_hip.h")) as f:
        header = f.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gnc_[a-z0-9_]+)", nm))
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported
    assert re.search(r"#define\s+GNC_PAD_BATCH_MAX_GRAPHS\s+64\b", header)
    assert native.PAD_BATCH_MAX_GRAPHS == 64
    # added without an ABI bump
    assert lib.gnc_abi_version() == 20 and native.ABI_VERSION == 20 and re.search(r"#define\s+GNC_ABI_VERSION\s+20\b", header)


def test_supported_query_answers_without_a_gpu():
    from graphnet_classifier_amd import native
    ok = native.pad_graph_batch_supported
    assert ok(64, 64 * 9, 64 * 40, 1024, 4096) and not ok(65, 65 * 9, 65 * 40, 1024, 4096)
    assert ok(1, 9, 40, 9, 40) and ok(3, 37, 180, 64, 256, 5, 2)
    assert not ok(0, 0, 0, 64, 256)
    assert not ok(3, 65, 180, 64, 256) and not ok(3, 37, 257, 64, 256)  # above a capacity
    assert ok(3, 64, 256, 64, 256)                                      # exactly at both
    assert ok(2, 12, 0, 32, 256)                                        # a batch without edges
    assert not ok(3, 37, 180, 64, 256, 0, 2) and not ok(3, 37, 180, 64, 256, 3, 0)
    assert not ok(3, 37, 180, 1 << 31, 256)                             # node ids are int32 inside the engine


@pytest.mark.parametrize("M,C,rows,D", [(64, 256, 96, 32), (64, 1, 65, 1), (64, 0, 65, 1), (37, 180, 60, 23), (32, 8, 33, 1),
                                        (32, 9, 34, 2), (1024, 4096, 1536, 512)])
def test_ragged_batch_layout(M, C, rows, D):
    """D = max(1, ceil(C / 8)) dummy nodes behind the M node slots."""
    from graphnet_classifier_amd import native
    assert native.ragged_batch_layout(M, C) == (rows, D)
    assert D == max(1, -(-C // 8)) and rows == M + D


def test_a_captured_batch_capacity_is_a_fixed_point_of_padded_capacity():
    """What ``train()`` captures at: edges in steps of 256, nodes in steps of 32; every batch that fits keeps the capacity (no
    re-capture), a batch above it grows it, and it never shrinks."""
    from graphnet_classifier_amd.train import padded_capacity
    for nodes, edges in ((37, 180), (256, 1400), (1, 0), (1200, 6900)):
        M, C = padded_capacity(nodes, 0, 32), padded_capacity(edges)
        assert M >= nodes and C >= edges and M % 32 == 0 and C % 256 == 0
        for n in (0, nodes, M):
            assert padded_capacity(n, M, 32) == M
        for e in (0, edges, C):
            assert padded_capacity(e, C) == C
        assert padded_capacity(M + 1, M, 32) > M and padded_capacity(C + 1, C) > C
        assert padded_capacity(M, padded_capacity(M + 1, M, 32), 32) == padded_capacity(M + 1, M, 32)


def test_new_names_are_importable():
    from graphnet_classifier_amd import GNN, train
    assert issubclass(train.CapturedRaggedBatchStep, train.CapturedTrainStep)
    assert issubclass(GNN.CapturedRaggedBatchForward, GNN.CapturedForward)
    assert hasattr(GNN.CombinedModel, "forward_batched_device")


class _FakeCapture:
    """What ``train._RaggedBatchCaptures`` reads of a capture object."""

    def __init__(self, batch, edge_capacity, node_capacity, log):
        from types import SimpleNamespace
        self.num_graphs, self.edge_capacity, self.node_capacity, self.log = batch.num_graphs, edge_capacity, node_capacity, log
        self.feed = SimpleNamespace(feature_shapes=(tuple(batch.x.shape[1:]), tuple(batch.pos.shape[1:])))
        log.append(("capture", node_capacity, edge_capacity))

    def matches(self, b):
        return b.num_graphs == self.num_graphs and b.num_nodes <= self.node_capacity and b.num_edges <= self.edge_capacity

    def check(self):
        self.log.append(("check", self.node_capacity, self.edge_capacity))


def test_ragged_batch_capture_policy_on_the_host():
    """Who gets a capture: the second of two batches with one graph count and different topologies; capacities only grow; the old
    capture is checked before it is replaced; with no capture left the old one stays and only the oversize batch runs eagerly; a
    short batch and a repeated topology run as before."""
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.train import _RaggedBatchCaptures
    log = []
    policy = _RaggedBatchCaptures(object(), lambda batch, **cap: _FakeCapture(batch, cap["edge_capacity"], cap["node_capacity"], log), limit=2)
    assert policy.allowed is False  # not a CombinedModel
    shapes = ((3, 3), (3, 4), (4, 4))
    a, b = synthetic.superpixel_like_graphs(3, 208, shapes=shapes), synthetic.superpixel_like_graphs(3, 207, shapes=shapes)  # 48, 27 nodes
    prev = (a.x, a.pos, a.edge_index, a.graph_ptr)
    assert policy.get(b, prev) is None and log == []
    policy.allowed = True
    assert policy.get(a, None) is None                     # no batch before it
    assert policy.get(a, prev) is None                     # the previous batch's topology: the fixed-topology capture's case
    short = synthetic.superpixel_like_graphs(2, 5, shapes=shapes)
    assert policy.get(short, prev) is None                 # another graph count
    wide = synthetic.superpixel_like_graphs(3, 207, shapes=shapes)
    wide.x = wide.x.repeat(1, 2)
    assert policy.get(wide, prev) is None and log == []    # other feature widths
    cap = policy.get(b, prev)
    assert cap is not None and log == [("capture", 96, 512)]          # 48 nodes / 198 edges, half as much again, quanta 32 / 256
    assert policy.get(a, None) is cap and policy.get(b, None) is cap  # both fit: no new capture, whatever ran before
    assert policy.get(short, None) is None and policy.current is cap  # a short last batch runs eagerly, the capture stays
    big = synthetic.superpixel_like_graphs(3, 5, shapes=((6, 6),))    # 108 nodes, above the node capacity
    cap2 = policy.get(big, None)
    assert cap2 is not cap and log[1] == ("check", 96, 512) and log[2][0] == "capture"
    assert cap2.node_capacity == 192 and cap2.edge_capacity >= big.num_edges and cap2.edge_capacity >= 512  # only grow
    huge = synthetic.superpixel_like_graphs(3, 5, shapes=((9, 9),))   # 243 nodes; both captures are used up
    assert policy.get(huge, None) is None and policy.current is cap2 and len(log) == 3
    assert policy.get(a, None) is cap2                                # ... and still serves what fits
    policy.check()
    assert log[-1][0] == "check"
