"""Routing of the fused MLP (K4 forward, K8 backward), no GPU: the 14 shape queries answer every description of
tests/mlp_route_cases.py exactly as recorded in tests/golden/mlp_routes.json - return codes as zero / nonzero, counts as
integers - with no switch set and with each A/B switch of the two routers set in a process of its own."""
import json
import os

import pytest

from tests import mlp_route_cases as C
from tests.golden import make_mlp_routes_golden as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_routes.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        stored = json.load(f)
    tables = C.unpack(stored)
    return {**stored, **tables.pop("no switch"), "switches": tables}


def _first_difference(got, want, stride=1):
    """Index, description and both answer vectors of the first case that differs (None when the tables agree)."""
    gv, gi = got["vectors"], got["index"]
    wv, wi = want["vectors"], want["index"]
    assert len(gi) == len(wi), (len(gi), len(wi))
    for k, (a, b) in enumerate(zip(gi, wi)):
        if gv[a] != wv[b]:
            names = [q for q, (x, y) in zip((n for n, _, _ in C.QUERIES), zip(gv[a], wv[b])) if x != y]
            return {"case": k * stride, "queries": names, "got": gv[a], "want": wv[b]}
    return None


def test_every_query_answers_as_recorded(golden):
    from graphnet_classifier_amd import native
    assert not any(s in os.environ for s in C.SWITCHES), "a routing switch is set in this environment"
    lib = native.load_library()
    assert golden["queries"] == [name for name, _, _ in C.QUERIES]
    assert golden["small_batch_max_rows"] == int(lib.gnc_mlp_small_batch_max_rows())
    vectors, index = C.answers(native, lib)
    assert _first_difference({"vectors": vectors, "index": index}, golden) is None


def test_the_recorded_table_shows_every_outcome_and_family(golden):
    """The table is only a proof if it reaches everything: both outcomes of each query, and every backward family,
    recognised by the answers that only that family gives."""
    reached = [golden["vectors"][k] for k in sorted(set(golden["index"]))]  # with no switch set
    col = {name: [v[q] for v in reached] for q, name in enumerate(golden["queries"])}
    for name, values in col.items():
        assert len(set(values)) >= 2, name
    assert any(v > 0 for v in col["gnc_mlp_backward_fused_rows"])                    # fused
    assert any(v == 1 for v in col["gnc_mlp_backward_small_batch_supported"])         # col16
    rows = set(col["gnc_mlp_backward_ln_partial_rows"])
    assert len(rows) >= 6, rows  # col16, col16-persist, resident, stream32 (2- and 8-wave), stream16 count differently
    # each backward switch changes answers on its thinned grid (the two forward ones move launches between kernels that
    # answer the queries alike: the GPU suites cover those)
    base = [golden["vectors"][k] for k in golden["index"][::C.SWITCH_STRIDE]]
    for s in C.SWITCHES[:6]:
        t = golden["switches"][s]
        assert any(t["vectors"][k] != b for k, b in zip(t["index"], base)), s


def test_every_switch_answers_as_recorded(golden):
    got = G.switch_tables()
    assert sorted(got) == sorted(golden["switches"]) == sorted(C.SWITCHES)
    for s in C.SWITCHES:
        assert _first_difference(got[s], golden["switches"][s], C.SWITCH_STRIDE) is None, s
        assert got[s]["index"] and len(got[s]["index"]) == len(golden["switches"][s]["index"])
