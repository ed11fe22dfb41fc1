"""Inputs and float64 references of the batched read-out tests (tests/test_gpu_readout_batched.py on the GPU,
tests/test_minibatch_host.py for the seed check on the host).  A case is built once per process and shared.

``y`` standard-normal, ``nn.Linear`` default initialisation at widths 128 / 32 / C, ``grad_logits`` standard-normal, all drawn
from ``torch.manual_seed(seed)`` in that order.  The reference is ``oracle.classifier_forward`` per graph in float64
(``oracle.to_dtype``) on features assembled by the gather rule on the CPU, its gradients float64 autograd.

A ReLU whose float64 pre-activation lies within 1e-5 of zero may legitimately come out on the other side in fp32, which moves
a gradient by a whole weight column.  No graph is excused for that: the seeds below are chosen - from the float64 oracle alone -
so that no case has a ``|z1|`` or ``|z2|`` below 1e-5, and ``test_minibatch_host`` asserts it."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import torch

from oracle import graphnet_oracle as O

H1, H2 = 128, 32
FLIP_MARGIN = 1e-5


@dataclass(frozen=True)
class Case:
    name: str
    num_nodes: int
    out_dim: int
    sizes: tuple          # nodes per graph
    classes: int = 2
    seed: int = 1
    use_graph_ptr: bool = True

    @property
    def num_graphs(self) -> int:
        return len(self.sizes)

    @property
    def features(self) -> int:
        return self.num_nodes * self.out_dim


CASES = (
    Case("single_graph", 36, 1, (36,), use_graph_ptr=False),
    Case("smaller_equal_larger", 156, 1, (144, 156, 169, 156, 144)),
    Case("out_dim3_partial_tile_F150", 50, 3, (50,) * 17, seed=2, use_graph_ptr=False),
    Case("two_tiles_plus_one_odd_F", 257, 1, (257,) * 33, use_graph_ptr=False),
    Case("several_F_slices", 1028, 1, (1028,) * 8, use_graph_ptr=False),
    Case("equal_via_num_graphs", 160, 1, (160,) * 40, seed=3, use_graph_ptr=False),
    Case("equal_via_graph_ptr", 160, 1, (160,) * 40, seed=3, use_graph_ptr=True),
    Case("three_classes_ragged_out_dim2", 20, 2, (25, 20, 7), classes=3),
    # 16 graphs per workgroup of the tail launch (G >= 256) and several graph ranges behind dW1
    Case("tail_tiles", 10, 1, (10,) * 300, seed=4, use_graph_ptr=False),
)
BY_NAME = {c.name: c for c in CASES}


def gather_features(y: torch.Tensor, graph_ptr: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """[G, num_nodes * out_dim]: feature k * out_dim + j of graph g is y[start_g + k, j] for k < min(size_g, num_nodes), else 0."""
    rows = []
    for g in range(graph_ptr.numel() - 1):
        s, e = int(graph_ptr[g]), int(graph_ptr[g + 1])
        k = min(e - s, num_nodes)
        rows.append(torch.cat([y[s:s + k], y.new_zeros(num_nodes - k, y.size(1))]).flatten())
    return torch.stack(rows)


@functools.lru_cache(maxsize=None)
def build(name: str) -> dict:
    """Inputs (float32, CPU) and the float64 reference of a case: ``logits``, ``grads`` (dy, dW1, db1, dW2, db2, dW3, db3),
    ``min_preact`` = the smallest ``|z1|`` / ``|z2|`` of the float64 oracle.  Read-only: shared between tests."""
    c = BY_NAME[name]
    torch.manual_seed(c.seed)
    graph_ptr = torch.tensor([0] + list(torch.tensor(c.sizes).cumsum(0)), dtype=torch.int64)
    y = torch.randn(int(graph_ptr[-1]), c.out_dim)
    fc1, fc2, fc3 = torch.nn.Linear(c.features, H1), torch.nn.Linear(H1, H2), torch.nn.Linear(H2, c.classes)
    grad = torch.randn(c.num_graphs, c.classes)
    sd = {f"classifier.{n}.{p}": getattr(m, p).detach().clone() for n, m in (("fc1", fc1), ("fc2", fc2), ("fc3", fc3))
          for p in ("weight", "bias")}
    sd64 = {k: v.requires_grad_(True) for k, v in O.to_dtype(sd, torch.float64).items()}
    y64 = y.double().requires_grad_(True)
    feats = gather_features(y64, graph_ptr, c.num_nodes)
    logits = torch.stack([O.classifier_forward(sd64, feats[g]) for g in range(c.num_graphs)])
    (logits * grad.double()).sum().backward()
    with torch.no_grad():
        z1 = O.linear(feats, sd64["classifier.fc1.weight"], sd64["classifier.fc1.bias"])
        z2 = O.linear(z1.clamp_min(0), sd64["classifier.fc2.weight"], sd64["classifier.fc2.bias"])
    order = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
    grads = (y64.grad,) + tuple(sd64["classifier." + k].grad for k in order)
    return {"case": c, "y": y, "graph_ptr": graph_ptr, "sd": sd, "grad_logits": grad, "logits": logits.detach(), "grads": grads,
            "grad_names": ("dy", "dW1", "db1", "dW2", "db2", "dW3", "db3"),
            "min_preact": float(min(z1.abs().min(), z2.abs().min()))}
