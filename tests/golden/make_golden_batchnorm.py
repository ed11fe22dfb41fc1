#!/usr/bin/env python3
"""Capture the norm_type='BatchNorm1d' golden vectors by running the REFERENCE's own classes on the CPU.

Run in the build container only (needs the reference checkout ``make_golden.py`` names):

    python tests/golden/make_golden_batchnorm.py

Writes tests/golden/g11_batchnorm.npz (data only: inputs, explicit weights, expected outputs).  Two cases:

* ``w16``: GraphNet(norm_type='BatchNorm1d', n_blocks=2, all widths 16) on a random graph with N = 37, E = 211;
* ``w64``: all widths 64, n_blocks=1, N = 150, E = 900 (the width class of the weights-resident kernels);

each wrapped in CombinedModel(num_nodes=N, classes=2).  Per case, from ONE training-mode forward + backward of the reference
(utils/train_model.py:37-41 without the optimizer step): the state dict before it, the inputs, the per-node GraphNet output,
the logits, the cross-entropy loss, every parameter gradient, every buffer (running_mean / running_var / num_batches_tracked)
after it, and the eval-mode GraphNet output and logits computed afterwards from those buffers.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, _np, _register_metalayer, _save, _sd, random_graph  # noqa: E402

CASES = (("w16", 16, 2, 37, 211, 11), ("w64", 64, 1, 150, 900, 12))


def kwargs(width, n_blocks):
    return dict(num_local_features=3, space_dim=2, out_channels=1, n_blocks=n_blocks, out_dim_node=width, out_dim_edge=width,
                hidden_dim_node=width, hidden_dim_edge=width, hidden_dim_decoder=width, hidden_dim_processor_node=width,
                hidden_dim_processor_edge=width, norm_type="BatchNorm1d")


def main():
    sys.path.insert(0, REF)
    _register_metalayer()
    from models.GNN import CombinedModel, GraphNet

    arrays = {}
    for tag, width, n_blocks, n, e, seed in CASES:
        rng = np.random.default_rng(seed)
        torch.manual_seed(seed)
        kw = kwargs(width, n_blocks)
        model = CombinedModel(GraphNet(**kw), num_nodes=n, classes=2)
        with torch.no_grad():  # non-trivial affine so gamma / beta are exercised
            for m in model.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.5, 0.5)
        ei = torch.from_numpy(random_graph(rng, n, e))
        x = torch.rand(n, 3)
        pos = torch.rand(n, 2) * 32
        label = torch.tensor(1)
        arrays.update(_sd(model, f"{tag}/sd/"))
        arrays[f"{tag}/kwargs_json"] = np.frombuffer(repr(kw).encode(), dtype=np.uint8)
        arrays.update({f"{tag}/x": _np(x), f"{tag}/pos": _np(pos), f"{tag}/edge_index": _np(ei), f"{tag}/label": _np(label)})
        kept = {}
        hook = model.graph_net.register_forward_hook(lambda mod, inp, out: kept.__setitem__("y", out.detach().clone()))
        model.train()
        logits = model(x, pos, ei)
        loss = torch.nn.CrossEntropyLoss()(logits, label)
        loss.backward()
        arrays.update({f"{tag}/train_y": _np(kept["y"]), f"{tag}/train_logits": _np(logits), f"{tag}/loss": _np(loss)})
        arrays.update({f"{tag}/grad/{k}": _np(p.grad) for k, p in model.named_parameters()})
        arrays.update({f"{tag}/after/{k}": _np(b) for k, b in model.named_buffers()})
        model.eval()
        with torch.no_grad():
            eval_logits = model(x, pos, ei)
        arrays.update({f"{tag}/eval_y": _np(kept["y"]), f"{tag}/eval_logits": _np(eval_logits)})
        hook.remove()
    _save("g11_batchnorm.npz", **arrays)


if __name__ == "__main__":
    main()
