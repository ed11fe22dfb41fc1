"""Host-only checks behind mini-batch training: the loader's index batches against ``torch.utils.data.DataLoader``, the batched
read-out's ``supported`` query (no GPU), the seeds of the GPU read-out cases (no float64 pre-activation near a ReLU's zero), and
``collate_graphs`` on CPU tensors."""
import itertools

import pytest
import torch
from torch.utils.data import DataLoader

from tests import readout_batched_cases as R


class _Folder:
    """What ``GraphFolderLoader.index_batches`` reads of a dataset: its length."""

    def __init__(self, n):
        self.samples = [(f"img{i}.png", i % 2) for i in range(n)]

    def __len__(self):
        return len(self.samples)


@pytest.mark.parametrize("batch_size,shuffle,drop_last", list(itertools.product((1, 3, 4), (False, True), (False, True))))
def test_index_batches_are_the_dataloaders(batch_size, shuffle, drop_last):
    from graphnet_classifier_amd.dataset import GraphFolderLoader
    n = 10
    loader = GraphFolderLoader(_Folder(n), shuffle=shuffle, batch_size=batch_size, drop_last=drop_last)
    for seed in (0, 1234):
        torch.manual_seed(seed)
        ref = [b.tolist() for b in DataLoader(range(n), batch_size=batch_size, shuffle=shuffle, drop_last=drop_last)]
        ref2 = [b.tolist() for b in DataLoader(range(n), batch_size=batch_size, shuffle=shuffle, drop_last=drop_last)]  # a second epoch
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        got, got2 = loader.index_batches(), loader.index_batches()
        assert got == ref and got2 == ref2
        assert torch.equal(torch.get_rng_state(), state)  # the same draws from the global generator
        assert len(loader) == len(ref)
    if batch_size == 1:  # the per-sample order is what it was
        torch.manual_seed(5)
        flat = loader.order()
        torch.manual_seed(5)
        assert [b[0] for b in loader.index_batches()] == flat


def test_loader_rejects_a_batch_size_below_one():
    from graphnet_classifier_amd.dataset import GraphFolderLoader
    with pytest.raises(ValueError):
        GraphFolderLoader(_Folder(4), batch_size=0)


def test_readout_batched_supported_answers_without_a_gpu():
    from graphnet_classifier_amd import native
    assert "gnc_readout_batched_supported" in native.EXPORTED_SYMBOLS
    for c in R.CASES:
        plan = native.readout_batched_plan(c.num_graphs, c.features, R.H1, R.H2, c.classes)
        assert plan is not None, c.name
        assert native.readout_batched_supported(c.num_graphs, c.features, R.H1, R.H2, c.classes)
        assert plan["f_slice_len"] % 32 == 0 and plan["f_slices"] * plan["f_slice_len"] >= c.features
        assert (plan["f_slices"] - 1) * plan["f_slice_len"] < c.features           # no empty slice
        assert plan["dw1_parts"] * plan["dw1_graph_range"] >= c.num_graphs and plan["dw1_graph_range"] % 16 == 0
        assert plan["forward_workspace_floats"] == plan["f_slices"] * c.num_graphs * R.H1
        assert plan["backward_workspace_floats"] >= c.num_graphs * R.H1
    # the two regimes the split is chosen for: thousands of graphs -> the graph tiles are the parallelism, a handful of graphs at
    # the reference's 128 x 128 pixel graph -> the F split is
    assert native.readout_batched_plan(6250, 160, 128, 32, 2)["f_slices"] == 1
    assert native.readout_batched_plan(8, 16384, 128, 32, 2)["f_slices"] >= 64
    assert native.readout_batched_supported(8, 16384, 128, 32, 64) and native.readout_batched_supported(3, 1, 128, 1, 1)
    assert not native.readout_batched_supported(8, 100, 2000, 32, 2)             # H1 = 2000
    assert native.readout_batched_plan(8, 100, 2000, 32, 2) is None
    assert not native.readout_batched_supported(8, 100, 128, 33, 2) and not native.readout_batched_supported(8, 100, 128, 32, 65)
    assert not native.readout_batched_supported(0, 100, 128, 32, 2) and not native.readout_batched_supported(8, 0, 128, 32, 2)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_no_float64_preactivation_of_the_gpu_cases_is_near_a_relu_zero(name):
    ref = R.build(name)
    print(f"{name}: min |z1|, |z2| = {ref['min_preact']:.3e}")
    assert ref["min_preact"] >= R.FLIP_MARGIN
    c = ref["case"]
    assert ref["logits"].shape == (c.num_graphs, c.classes) and ref["grads"][1].shape == (R.H1, c.features)


def test_collate_graphs_round_trips_through_slice_graphs():
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.image_to_graph import collate_graphs
    src = synthetic.superpixel_like_graphs(4, seed=3)
    graphs = []
    for g in range(4):
        b = src.slice_graphs(g, g + 1)
        graphs.append((b.x, b.pos, b.edge_index))
    batch = collate_graphs(graphs)
    assert isinstance(batch, synthetic.GraphBatch) and batch.num_graphs == 4
    assert torch.equal(batch.graph_ptr, src.graph_ptr) and torch.equal(batch.edge_ptr, src.edge_ptr)
    assert torch.equal(batch.x, src.x) and torch.equal(batch.pos, src.pos) and torch.equal(batch.edge_index, src.edge_index)
    assert batch.edge_index.dtype == torch.int64 and batch.graph_ptr.dtype == torch.int64
    for g, (x, pos, ei) in enumerate(graphs):
        b = batch.slice_graphs(g, g + 1)
        assert torch.equal(b.x, x) and torch.equal(b.pos, pos) and torch.equal(b.edge_index, ei)
    one = collate_graphs(graphs[:1])
    assert torch.equal(one.edge_index, graphs[0][2]) and one.graph_ptr.tolist() == [0, graphs[0][0].size(0)]
    with pytest.raises(ValueError):
        collate_graphs([])
