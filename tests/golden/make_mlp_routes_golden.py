"""Records tests/golden/mlp_routes.json: the answers of the 14 fused-MLP shape queries over tests/mlp_route_cases.py.

Run it against the library whose routing is to be pinned (GNC_LIB_PATH names a build other than the in-tree one), before the
routing code changes:

    GNC_LIB_PATH=/path/to/parent/libgnc_hip.so python tests/golden/make_mlp_routes_golden.py

The file holds each distinct answer vector once and one index per case in enumeration order (deflated, base64:
tests/mlp_route_cases.py pack / unpack); each A/B switch is recorded on a
thinned grid in a child process of its own (the library reads a switch once per process)."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import mlp_route_cases as C  # noqa: E402


def switch_tables():
    """{switch: table of the thinned grid with that switch set}, children run side by side."""
    env = {k: v for k, v in os.environ.items() if k not in C.SWITCHES}
    procs = {s: subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mlp_route_cases.py"), str(C.SWITCH_STRIDE)],
                                 env={**env, s: "1"}, stdout=subprocess.PIPE, text=True) for s in C.SWITCHES}
    out = {}
    for s, p in procs.items():
        text, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"child for {s} ended with {p.returncode}")
        out[s] = json.loads(text)
    return out


def main():
    from graphnet_classifier_amd import native
    assert not any(s in os.environ for s in C.SWITCHES), "record with no routing switch set"
    lib = native.load_library()
    vectors, index = C.answers(native, lib)
    for q, (name, _, _) in enumerate(C.QUERIES):  # every query must show each of its outcomes
        seen = {v[q] for v in vectors}
        assert len(seen) >= 2, (name, seen)
    table = {"queries": [name for name, _, _ in C.QUERIES], "small_batch_max_rows": int(lib.gnc_mlp_small_batch_max_rows()),
             **C.pack({"no switch": {"vectors": vectors, "index": index}, **switch_tables()})}
    path = os.path.join(HERE, "mlp_routes.json")
    with open(path, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(index)} cases, {len(vectors)} distinct answer vectors, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
