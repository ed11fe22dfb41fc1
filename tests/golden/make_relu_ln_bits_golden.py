#!/usr/bin/env python3
"""Record the bit fixtures of tests/test_gpu_relu_layernorm_bits.py from the library of the PARENT commit, on an MI355X.

The fixtures pin what the fused-MLP kernels computed BEFORE the ReLU of an accumulator became one instruction (DESIGN.md
K4), so they are worthless when written by the code under test: build the parent commit into its own object directory
and select that library with GNC_LIB_PATH (the procedure of tests/golden/make_split_bits_golden.py),

    (in a checkout of the parent)  make -C graphnet_classifier_amd/csrc OBJDIR=../../build/parent TARGET=../../build/libgnc_parent.so
    GNC_LIB_PATH=build/libgnc_parent.so python tests/golden/make_relu_ln_bits_golden.py --commit <parent hash> [--out DIR]

Writes into tests/golden/relu_ln_bits/ (or DIR): one ``<case>_<rows>.npz`` per case and row count of the test module
(tensors below 1,024 rows whole, larger ones as every 97th row) and ``relu_ln_bits.json`` with the commit, the command,
the library, and per case the kernel family that served it and the shape and SHA-256 of every full tensor."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "relu_ln_bits"))
    a = ap.parse_args()
    from graphnet_classifier_amd import native
    from tests import test_gpu_relu_layernorm_bits as m
    from tests.test_gpu_split_pipeline_bits import ROW_STEP, WHOLE_BELOW
    native.load_library()
    os.makedirs(a.out, exist_ok=True)
    lib = os.path.relpath(os.environ.get("GNC_LIB_PATH", native.LIB_PATH), ROOT)  # as named from the repository root
    meta = {"commit": a.commit, "command": "GNC_LIB_PATH=%s python tests/golden/make_relu_ln_bits_golden.py --commit %s" % (lib, a.commit),
            "library": lib, "device": torch.cuda.get_device_name(0), "row_step": ROW_STEP, "whole_below": WHOLE_BELOW, "cases": {}}
    for name, rows in m.KEYS:
        got, family = m.run_case(native, name, rows)
        np.savez_compressed(os.path.join(a.out, f"{name}_{rows}.npz"), **{k: m.stored_rows(v).numpy() for k, v in got.items()})
        meta["cases"][f"{name}/{rows}"] = {"family": family,
                                           "tensors": {k: {"shape": list(v.shape), "sha256": m.sha256(v)} for k, v in got.items()}}
        print(name, rows, family, sorted(got), flush=True)
    with open(os.path.join(a.out, "relu_ln_bits.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
