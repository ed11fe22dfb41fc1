"""Per-launch time of the batched read-out (csrc/readout_batched.hip) against the torch path it replaces (the gather / product that
materialises [G, F] in graph_ptr mode, three nn.Linear GEMMs, two clamps), forward and forward + backward, at the shapes of the
two regimes.  Prints one JSON line per shape and writes them to the file given as the first argument (default: stdout only).

    python tools/bench_readout_batched.py profiles/readout_batched.json
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphnet_classifier_amd import functional as Fn  # noqa: E402

DEV = "cuda:0"
SHAPES = [  # (label, graphs, num_nodes, sizes or None)
    ("c3: G=6250 F=160", 6250, 160, None),
    ("c2: G=10000 F=156 ragged 144/156/169", 10000, 156, (144, 156, 169)),
    ("pixel 128x128: G=8 F=16384", 8, 16384, None),
    ("pixel 128x128: G=64 F=16384", 64, 16384, None),
]


def torch_path(y, gp, G, num_nodes, w1, b1, w2, b2, w3, b3):
    if gp is None:
        feats = y.view(G, -1)
    else:
        start, size = gp[:-1], gp[1:] - gp[:-1]
        k = torch.arange(num_nodes, device=y.device)
        valid = k[None, :] < size[:, None]
        rows = (start[:, None] + k[None, :]).clamp_(max=max(y.size(0) - 1, 0))
        feats = (y[rows] * valid[..., None]).reshape(G, num_nodes * y.size(1))
    lin = torch.nn.functional.linear
    return lin(torch.relu(lin(torch.relu(lin(feats, w1, b1)), w2, b2)), w3, b3)


def timed(fn, warmup=10, reps=40):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms) * 1e3, min(ms) * 1e3  # microseconds


def main():
    rows = []
    for label, G, num_nodes, sizes in SHAPES:
        torch.manual_seed(0)
        if sizes is None:
            gp, n = None, G * num_nodes
        else:
            s = torch.tensor(sizes)[torch.randint(0, len(sizes), (G,))]
            gp = torch.cat([torch.zeros(1, dtype=torch.int64), s.cumsum(0)]).to(DEV)
            n = int(gp[-1])
        y = torch.randn(n, 1, device=DEV, requires_grad=True)
        fc = [torch.nn.Linear(num_nodes, 128), torch.nn.Linear(128, 32), torch.nn.Linear(32, 2)]
        params = [p.detach().to(DEV).requires_grad_(True) for m in fc for p in (m.weight, m.bias)]
        grad = torch.randn(G, 2, device=DEV)
        row = {"shape": label}
        for name, f in (("hip", Fn.readout_batched), ("torch", torch_path)):
            def fwd():
                with torch.no_grad():
                    f(y, gp, G, num_nodes, *params)

            def both():
                y.grad = None
                for p in params:
                    p.grad = None
                f(y, gp, G, num_nodes, *params).backward(grad)
            row[name + "_fwd_us"], _ = timed(fwd)
            row[name + "_fwd_bwd_us"], _ = timed(both)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
