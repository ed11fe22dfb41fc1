#!/usr/bin/env python3
"""Record the bit fixtures of tests/test_gpu_split_bits.py from the library of the PARENT commit, on an MI355X.

The fixtures pin what the weights-resident kernel's split class (3-way bf16 split) computed BEFORE a change
to its instruction stream, so they are worthless when written by the code under test: build the parent commit into its
own object directory and select that library with GNC_LIB_PATH,

    (in a checkout of the parent)  make -C graphnet_classifier_amd/csrc OBJDIR=../../build/parent TARGET=../../build/libgnc_parent.so
    GNC_LIB_PATH=build/libgnc_parent.so python tests/golden/make_split_bits_golden.py --commit <parent hash> [--out DIR]

Writes into tests/golden/split_bits/ (or DIR):

* ``graphnet_c3_004.npy``: the [40000, 1] output of GraphNet(**kw) (torch.manual_seed(0), eval, no_grad) on
  synthetic.make_workload("c3", 0.04) - 250 graphs, 40,000 nodes, 400,000 edges: every launch of the flagship forward on
  the resident split class (EF encoder, DUAL projection, storing and aggregate-only edge processor, node processors, decoder);
* ``mlp_edge_rows.npy`` / ``mlp_enc_rows.npy``: every 97th row of the two native.mlp_forward cases of
  tests/test_gpu_split_mlp.py (70,007 rows: waves walk more than one tile);
* ``split_bits.json``: the commit, the command, the library, and the SHA-256 of each full output's bytes.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ROW_STEP = 97


def graphnet_output():
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import GraphNet
    from graphnet_classifier_amd.topology import clear_topology_cache
    batch, kw = synthetic.make_workload("c3", 0.04)
    torch.manual_seed(0)
    model = GraphNet(**kw).to("cuda").eval()
    clear_topology_cache()
    with torch.no_grad():
        y = model(batch.x.to("cuda"), batch.pos.to("cuda"), batch.edge_index.to("cuda"))
    torch.cuda.synchronize()
    return batch, y.cpu().numpy()


def mlp_output(kind):
    from graphnet_classifier_amd import native
    from tests import test_gpu_split_mlp as m
    out, _ = m._forward(native, kind, m._case(kind))
    return out.numpy()


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the selected library was built from (the parent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "split_bits"))
    a = ap.parse_args()
    from graphnet_classifier_amd import native
    native.load_library()
    os.makedirs(a.out, exist_ok=True)
    batch, y = graphnet_output()
    assert y.shape == (40000, 1) and y.dtype == np.float32, (y.shape, y.dtype)
    np.save(os.path.join(a.out, "graphnet_c3_004.npy"), y)
    lib = os.path.relpath(os.environ.get("GNC_LIB_PATH", native.LIB_PATH), ROOT)  # as named from the repository root
    meta = {"commit": a.commit, "command": "GNC_LIB_PATH=%s python tests/golden/make_split_bits_golden.py --commit %s" % (lib, a.commit),
            "library": lib, "device": torch.cuda.get_device_name(0), "row_step": ROW_STEP,
            "graphnet": {"workload": "c3", "scale": 0.04, "graphs": int(batch.num_graphs), "nodes": int(batch.num_nodes),
                         "edges": int(batch.num_edges), "sha256": sha256(y)},
            "mlp": {}}
    for kind in ("edge", "enc"):
        out = mlp_output(kind)
        np.save(os.path.join(a.out, f"mlp_{kind}_rows.npy"), out[::ROW_STEP])
        meta["mlp"][kind] = {"shape": list(out.shape), "sha256": sha256(out)}
    with open(os.path.join(a.out, "split_bits.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(meta))


if __name__ == "__main__":
    main()
