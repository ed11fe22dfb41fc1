"""Host-only checks behind the captured ragged-batch step: the feed launch's C ABI (``gnc_pad_graph_batch`` and its ``supported``
query, declared, exported, answered without a GPU), the buffer layout ``ragged_batch_layout``, the capacity rule, and the training
loop's capture decisions (``train._PaddedCaptures``, ``train._SampleStepper``) driven on the CPU with fake capture classes."""
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
    """What ``train._PaddedCaptures`` reads of a capture object."""

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
    from graphnet_classifier_amd.train import _PaddedCaptures
    log = []
    policy = _PaddedCaptures(object(), lambda batch, **cap: _FakeCapture(batch, cap["edge_capacity"], cap["node_capacity"], log), limit=2)
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


# --------------------------------------------------------------------------- the training loop's capture decisions, on the host
def _fake_capture_classes(log, calls):
    """Stand-ins for ``train.CapturedTrainStep`` / ``CapturedRaggedBatchStep`` / ``CapturedTensorStep``: no device, the real feeds'
    ``matches`` rules (``FixedGraphFeed`` / ``PaddedGraphFeed`` / ``RaggedBatchFeed`` / ``CapturedTensorStep``), every ``matches`` call
    counted in ``calls[0]`` and ``(event, kind, node_capacity, edge_capacity)`` appended to ``log`` per capture, replay and check."""
    import torch
    from types import SimpleNamespace

    class Fake:
        kind = node_capacity = edge_capacity = None

        def _log(self, event):
            log.append((event, self.kind, self.node_capacity, self.edge_capacity))

        def matches(self, *sample):
            calls[0] += 1
            return self._fits(*sample)

        def __call__(self, sample, label):
            assert self._fits(sample), "a replay of a sample the feed would refuse"
            self._log("replay")

        def check(self):
            self._log("check")

    class Step(Fake):
        def __init__(self, model, optimizer, criterion, sample, label, loss_sum, *, forward=None, edge_capacity=None, node_capacity=None):
            self.x, self.pos, self.given = sample
            self.num_nodes = int(self.x.size(0))
            self.edge_capacity, self.node_capacity = edge_capacity, node_capacity
            self.kind = "padded" if edge_capacity is not None else "fixed" if forward is None else "fixed_batch"
            assert self._fits(sample)
            self._log("capture")

        def _fits(self, sample):
            x, pos, edge_index = sample
            if self.edge_capacity is None:
                return (x.shape == self.x.shape and pos.shape == self.pos.shape and edge_index.shape == self.given.shape
                        and bool(torch.equal(edge_index, self.given)))
            nodes_fit = x.size(0) == self.num_nodes if self.node_capacity is None else x.size(0) <= self.node_capacity
            return (nodes_fit and x.shape[1:] == self.x.shape[1:] and pos.shape[1:] == self.pos.shape[1:]
                    and edge_index.dim() == 2 and edge_index.size(1) <= self.edge_capacity)

        def __call__(self, sample, label):
            super().__call__(sample, label)
            if self.node_capacity is not None:
                self.num_nodes = int(sample[0].size(0))

    class RaggedBatchStep(Fake):
        kind = "ragged_batch"

        def __init__(self, model, optimizer, criterion, batch, labels, loss_sum, *, edge_capacity, node_capacity):
            self.num_graphs, self.edge_capacity, self.node_capacity = batch.num_graphs, edge_capacity, node_capacity
            self.feed = SimpleNamespace(feature_shapes=(tuple(batch.x.shape[1:]), tuple(batch.pos.shape[1:])))
            assert self._fits(batch)
            self._log("capture")

        def _fits(self, b):
            return (b.num_graphs == self.num_graphs and b.x.size(0) <= self.node_capacity and b.edge_index.size(1) <= self.edge_capacity
                    and (tuple(b.x.shape[1:]), tuple(b.pos.shape[1:])) == self.feed.feature_shapes)

    class TensorStep(Fake):
        kind = "tensor"

        def __init__(self, model, optimizer, criterion, sample, label, loss_sum):
            self.x, self.label = sample, torch.as_tensor(label)
            self._log("capture")

        def _fits(self, sample, label=None):
            return (isinstance(sample, torch.Tensor) and sample.shape == self.x.shape and sample.dtype == self.x.dtype
                    and (label is None or torch.as_tensor(label).shape == self.label.shape))

        def __call__(self, sample, label):
            assert self._fits(sample, label)
            self._log("replay")

    return Step, RaggedBatchStep, TensorStep


def _host_stepper(monkeypatch, model, log, calls):
    """A real ``train._SampleStepper`` on the CPU over ``model``: fake capture classes, a no-op optimizer."""
    import torch
    from types import SimpleNamespace
    from graphnet_classifier_amd import train
    step, ragged, tensor = _fake_capture_classes(log, calls)
    monkeypatch.setattr(train, "CapturedTrainStep", step)
    monkeypatch.setattr(train, "CapturedRaggedBatchStep", ragged)
    monkeypatch.setattr(train, "CapturedTensorStep", tensor)
    optimizer = SimpleNamespace(zero_grad=lambda: None, step=lambda: None)
    return train._SampleStepper(model, optimizer, torch.nn.CrossEntropyLoss(), torch.zeros((), dtype=torch.float64),
                                torch.device("cpu"), True)


def _fake_model(log, num_nodes, ragged_readout=False, pooling=False):
    """What the stepper reads of a ``CombinedModel``; the eager forwards log which form ran."""
    import torch
    from torch import nn

    class FakeModel(nn.Module):
        def __init__(self):
            super().__init__()
            self.graph_net, self.classifier = nn.Identity(), nn.Identity()
            self.graph_net.pooling = pooling
            self.num_nodes, self.ragged_readout = num_nodes, ragged_readout
            self.w = nn.Parameter(torch.zeros(2))

        def forward(self, sample):
            log.append(("eager", "graph", None, None))
            return self.w + sample[0].sum()

        def forward_batched(self, x, pos, edge_index, num_graphs=None, graph_ptr=None):
            if graph_ptr is None:  # CombinedModel.forward_batched's own conditions for the num_graphs form
                if x.size(0) != num_graphs * self.num_nodes or self.graph_net.pooling:
                    raise ValueError("pass graph_ptr")
            log.append(("eager", "num_graphs" if graph_ptr is None else "graph_ptr", None, None))
            graphs = num_graphs if graph_ptr is None else graph_ptr.numel() - 1
            return self.w.expand(graphs, 2) + x.sum()

    return FakeModel()


def _drive(stepper, log, calls, samples):
    """Steps ``samples`` ([(sample, label)]); per sample ``(the events it logged, the matches calls it made)``.  The tests below
    hold the events to the recorded decisions and the calls to no more than the loop made when they were recorded."""
    out = []
    for sample, label in samples:
        del log[:]
        calls[0] = 0
        stepper(sample, label)
        out.append((list(log), calls[0]))
    return out


def _graph(nodes, edges, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(nodes, 3, generator=g), torch.rand(nodes, 2, generator=g), torch.randint(0, nodes, (2, edges), generator=g)),
            torch.tensor(seed % 2))


def _captured(kind, nodes, edges):
    return [("capture", kind, nodes, edges), ("replay", kind, nodes, edges)]


EAGER_GRAPH = [("eager", "graph", None, None)]
SINGLE_GRAPHS = ((64, 200, 1), (64, 200, 1), (64, 210, 2), (64, 180, 3), (64, 200, 1), (64, 400, 4), (64, 700, 5), (64, 1200, 6),
                 (64, 2000, 7), (64, 3000, 8), (64, 190, 9), (64, 3000, 8), (48, 100, 10))
SINGLE_GRAPHS_RAGGED = ((80, 300, 11), (40, 100, 12), (200, 300, 13), (64, 210, 2))


@pytest.mark.parametrize("ragged_readout", [False, True])
def test_single_graph_capture_decisions_on_the_host(monkeypatch, ragged_readout):
    """A stream of single graphs through the training loop's stepper: a repeated topology gets its own fixed capture, a new
    one the padded capture, which grows (512 -> 1280 -> 3072 edge slots) as samples outgrow it - checked before it is replaced.
    Another node count runs eagerly on a model without ``ragged_readout``; with it the capture takes the node-capacity form, which
    keeps the 3072 edge slots and serves the 64-node graphs too (96 node slots).  That is the fourth and last capture: the
    200-node graph runs eagerly on its own, the capture stays for what fits and the final check reaches it."""
    log, calls = [], [0]
    stepper = _host_stepper(monkeypatch, _fake_model(log, 64, ragged_readout), log, calls)
    sequence = SINGLE_GRAPHS + (SINGLE_GRAPHS_RAGGED if ragged_readout else ())
    trace = _drive(stepper, log, calls, [_graph(*s) for s in sequence])
    replay = lambda n, e: [("replay", "padded", n, e)]  # noqa: E731
    expected = [
        (EAGER_GRAPH, 0),
        (_captured("fixed", None, None), 1),
        (_captured("padded", None, 512), 2),
        (replay(None, 512), 3),
        ([("replay", "fixed", None, None)], 1),
        (replay(None, 512), 3),
        ([("check", "padded", None, 512)] + _captured("padded", None, 1280), 3),
        (replay(None, 1280), 3),
        ([("check", "padded", None, 1280)] + _captured("padded", None, 3072), 3),
        (replay(None, 3072), 3), (replay(None, 3072), 3), (replay(None, 3072), 3)]
    if not ragged_readout:
        expected += [(EAGER_GRAPH, 3)]
        final = [("check", "padded", None, 3072)]
    else:
        expected += [([("check", "padded", None, 3072)] + _captured("padded", 96, 3072), 3), (replay(96, 3072), 3), (replay(96, 3072), 3),
                     (EAGER_GRAPH, 2), (replay(96, 3072), 2)]  # (the replay asks the fixed capture, then the padded one)
        final = [("check", "padded", 96, 3072)]
    for k, ((events, count), (want, most)) in enumerate(zip(trace, expected), 1):
        assert events == want and count <= most, (k, events, count)
    assert len(trace) == len(expected)
    del log[:]
    stepper.check()
    assert log == final


@pytest.mark.parametrize("capture_ragged_batches", [True, False])
def test_mini_batch_capture_decisions_on_the_host(monkeypatch, capture_ragged_batches):
    """Mini-batches through the stepper: the fixed-batch capture for a batch that repeats, the ragged capture for batches of one
    graph count (checked before it is replaced by a larger one), the eager step for a short batch - and for every ragged batch
    with ``capture_ragged_batches`` off."""
    import torch
    from graphnet_classifier_amd import synthetic
    log, calls = [], [0]
    stepper = _host_stepper(monkeypatch, _fake_model(log, 64, True), log, calls)
    stepper.ragged.allowed = True  # (the rule asks for a CombinedModel)
    stepper.capture_ragged_batches = capture_ragged_batches

    def batch(graphs, seed, shapes=((3, 3), (3, 4), (4, 4))):
        return synthetic.superpixel_like_graphs(graphs, seed, shapes=shapes), torch.zeros(graphs, dtype=torch.int64)

    a, b, short, c, big = batch(3, 208), batch(3, 207), batch(2, 5), batch(3, 206), batch(3, 5, ((6, 6),))  # big: 108 nodes
    trace = _drive(stepper, log, calls, [a, a, b, short, a, c, big, short])
    eager = [("eager", "graph_ptr", None, None)]
    fixed = [("replay", "fixed_batch", None, None)]
    if capture_ragged_batches:
        expected = [(eager, 0), (_captured("fixed_batch", None, None), 1), (_captured("ragged_batch", 96, 512), 0), (eager, 1),
                    (fixed, 1), ([("replay", "ragged_batch", 96, 512)], 1),
                    ([("check", "ragged_batch", 96, 512)] + _captured("ragged_batch", 192, 512), 1), (eager, 1)]
        final = [("check", "ragged_batch", 192, 512)]
    else:
        expected = [(eager, 0), (_captured("fixed_batch", None, None), 1), (eager, 0), (eager, 0), (fixed, 1), (eager, 0), (eager, 0),
                    (eager, 0)]
        final = []
    for k, ((events, count), (want, most)) in enumerate(zip(trace, expected), 1):
        assert events == want and count <= most, (k, events, count)
    assert len(trace) == len(expected)
    del log[:]
    stepper.check()
    assert log == final


def test_eager_batch_step_takes_graph_ptr_behind_topk_pooling(monkeypatch):
    """A flatten read-out behind top-K pooling needs the graphs' offsets even when every graph has ``num_nodes`` nodes: the
    training step takes the ``graph_ptr`` form there, as ``evaluate`` does (``forward_batched(num_graphs=)`` raises ValueError)."""
    import torch
    from graphnet_classifier_amd import synthetic
    log, calls = [], [0]
    stepper = _host_stepper(monkeypatch, _fake_model(log, 16, pooling=True), log, calls)
    batch = synthetic.superpixel_like_graphs(3, 1, shapes=((4, 4),))
    assert _drive(stepper, log, calls, [(batch, torch.zeros(3, dtype=torch.int64))]) == [([("eager", "graph_ptr", None, None)], 0)]
    log, calls = [], [0]  # ... and without pooling the num_graphs form, as before
    stepper = _host_stepper(monkeypatch, _fake_model(log, 16), log, calls)
    assert _drive(stepper, log, calls, [(batch, torch.zeros(3, dtype=torch.int64))]) == [([("eager", "num_graphs", None, None)], 0)]


def test_tensor_capture_decisions_on_the_host(monkeypatch):
    """Plain tensor batches on this package's ``MLP``: captured when two consecutive batches share their shape; a short batch runs
    eagerly and the capture stays."""
    import torch
    from graphnet_classifier_amd.MLP import MLP
    log, calls = [], [0]

    def forward(self, x):
        log.append(("eager", "tensor", None, None))
        return self.model[0].weight.sum() + x.sum(dim=1, keepdim=True).expand(-1, 2)

    monkeypatch.setattr(MLP, "forward", forward)
    stepper = _host_stepper(monkeypatch, MLP(12, 2).cpu(), log, calls)  # (an MLP places itself on a GPU where one is visible)
    trace = _drive(stepper, log, calls, [(torch.rand(rows, 12), torch.zeros(rows, dtype=torch.int64)) for rows in (4, 4, 4, 3, 4)])
    eager, replay = [("eager", "tensor", None, None)], [("replay", "tensor", None, None)]
    assert trace == [(eager, 0), (_captured("tensor", None, None), 1), (replay, 1), (eager, 1), (replay, 1)]
