#!/usr/bin/env python3
"""Record the bit fixtures of tests/test_gpu_pool_family_bits.py from the library of the PARENT commit, on an MI355X.

The fixtures pin what the pooling kernels (K17, K19, K20) computed BEFORE they moved onto csrc/graph_reduce.h, so they are
worthless when written by the code under test: build the parent commit into its own object directory and select that library
with GNC_LIB_PATH (the procedure of tests/golden/make_relu_ln_bits_golden.py),

    (in a checkout of the parent)  make -C graphnet_classifier_amd/csrc OBJDIR=../../build/parent TARGET=../../build/libgnc_parent.so
    GNC_LIB_PATH=build/libgnc_parent.so python tests/golden/make_pool_family_bits_golden.py --commit <parent hash> [--out DIR]

Writes into tests/golden/pool_family_bits/ (or DIR): ``pool_family_bits.npz`` with every per-graph tensor, ``alpha`` and ``ds``
whole, under ``<family>/<batch>/<tensor>``, and ``pool_family_bits.json`` with the commit, the command, the library, the device
and per case the names of the whole tensors and the shape and SHA-256 of every [rows, C] tensor."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the selected library was built from (the parent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pool_family_bits"))
    a = ap.parse_args()
    from graphnet_classifier_amd import native
    from tests import test_gpu_pool_family_bits as m
    native.load_library()
    os.makedirs(a.out, exist_ok=True)
    lib = os.path.relpath(os.environ.get("GNC_LIB_PATH", native.LIB_PATH), ROOT)  # as named from the repository root
    meta = {"commit": a.commit, "command": "GNC_LIB_PATH=%s python tests/golden/make_pool_family_bits_golden.py --commit %s" % (lib, a.commit),
            "library": lib, "device": torch.cuda.get_device_name(0), "cases": {}}
    arrays = {}
    for family, batch in m.KEYS:
        whole, hashed = m.run_case(native, family, batch)
        arrays.update({f"{family}/{batch}/{k}": v.numpy() for k, v in whole.items()})
        meta["cases"][f"{family}/{batch}"] = {"whole": sorted(whole),
                                              "hashed": {k: {"shape": list(v.shape), "sha256": m.sha256(v)} for k, v in hashed.items()}}
        print(family, batch, len(whole), "whole,", len(hashed), "hashed", flush=True)
    np.savez_compressed(os.path.join(a.out, "pool_family_bits.npz"), **arrays)
    with open(os.path.join(a.out, "pool_family_bits.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
