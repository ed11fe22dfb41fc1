"""CPU checks of what carries the batched region-graph build and the ragged read-out: the two C symbols
(csrc/rag_batched.hip) and their supported set, the ``ragged_readout`` attribute, the capacity arithmetic."""
import os
import re

from graphnet_classifier_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gnc_rag_batched_workspace_bytes", "gnc_rag_build_batched")


def test_batched_rag_symbols_exported_at_abi_20():
    with open(os.path.join(ROOT, "include", "gnc_hip.h")) as f:
        header = f.read()
    lib = native.load_library()
    assert lib.gnc_abi_version() == 20 and native.ABI_VERSION == 20
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_workspace_query_is_the_supported_set():
    q = native.load_library().gnc_rag_batched_workspace_bytes
    assert q(64, 128, 128, 128, 1024) > 0
    assert q(1, 256, 256, 512, 4096) > 0
    assert q(1, 1, 1, 1, 1) > 0 and q(3, 96, 160, 200, 2048) > 0
    assert q(1, 0, 128, 128, 1024) == 0                    # H = 0
    assert q(1, 128, 128, 0, 1024) == 0                    # node_capacity = 0
    assert q(1, 128, 128, 513, 1024) == 0                  # capacities above the supported set
    assert q(1, 128, 128, 128, 4097) == 0
    assert q(1, 257, 256, 128, 1024) == 0 and q(0, 128, 128, 128, 1024) == 0
    assert b"supported set" in native.load_library().gnc_last_error_string()


def test_ragged_readout_is_a_plain_attribute():
    import torch
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    torch.manual_seed(0)
    model = CombinedModel(GraphNet(n_blocks=1, out_dim_node=8, out_dim_edge=8, hidden_dim_node=8, hidden_dim_edge=8,
                                   hidden_dim_decoder=8, hidden_dim_processor_node=8, hidden_dim_processor_edge=8),
                          num_nodes=10, classes=2)
    assert model.ragged_readout is False
    keys = list(model.state_dict())
    model.ragged_readout = True
    assert list(model.state_dict()) == keys and not any("ragged" in k for k in keys)
    assert {k.split(".")[0] for k in keys} == {"graph_net", "classifier"}


def test_superpixel_capacities_are_inside_the_supported_set():
    from graphnet_classifier_amd.image_to_graph import RAG_BATCHED_MAX_EDGES, RAG_BATCHED_MAX_NODES, superpixel_capacities
    q = native.load_library().gnc_rag_batched_workspace_bytes
    last = (0, 0)
    for n_segments in (1, 25, 64, 100, 128, 400, 1000, 5000):
        nodes, edges = superpixel_capacities(n_segments)
        assert 1 <= nodes <= RAG_BATCHED_MAX_NODES and 1 <= edges <= RAG_BATCHED_MAX_EDGES
        assert nodes >= min(n_segments, RAG_BATCHED_MAX_NODES) and (nodes, edges) >= last
        assert q(64, 128, 128, nodes, edges) > 0
        last = (nodes, edges)
    # the fixture graphs at the default parameters (69 - 119 nodes, 338 - 566 directed edges) and the largest one
    assert superpixel_capacities(100)[0] >= 119 and superpixel_capacities(100)[1] >= 566
    assert superpixel_capacities(400)[0] >= 423 and superpixel_capacities(400)[1] >= 1984


def test_padded_capacity_arithmetic():
    from graphnet_classifier_amd.train import padded_capacity
    for quantum in (32, 256):
        previous = 0
        for needed in range(0, 3000, 7):
            cap = padded_capacity(needed, 0, quantum)
            assert cap >= needed and cap % quantum == 0 and cap >= previous  # never below the size, monotone
            previous = cap
            for fits in (0, needed // 2, needed, cap):
                assert padded_capacity(fits, cap, quantum) == cap              # a fixed point for sizes that fit
            grown = padded_capacity(cap + 1, cap, quantum)
            assert grown > cap and grown >= cap + 1
    assert padded_capacity(566) == 1024 and padded_capacity(119, 0, 32) == 192
