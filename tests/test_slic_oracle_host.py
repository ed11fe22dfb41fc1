"""CPU: the licence of the sequential SLIC oracle (oracle/slic_oracle.py) and the conditions on the shape-case table
(tests/superpixel_shape_cases.py) that tests/test_gpu_superpixel_shapes.py compares the device SLIC with.

The oracle reproduces scikit-image 0.18.3's recorded labels of all 44 fixtures (tests/golden/g10_superpixel*.npz) bit
for bit; only then is it a reference at the shapes no fixture has.  The table's conditions are computed from the oracle
alone, so that the GPU comparison cannot pass on collapsed or all-emptied cases."""
import os
import re

import numpy as np
import pytest

from oracle import image_graph_oracle as IO
from oracle import slic_oracle
from tests import superpixel_shape_cases as S
from tests.test_superpixel_golden import CASES as FIXTURES

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphnet_classifier_amd", "csrc",
                   "superpixel.hip")


def kernel_centre_count(H, W, n_segments):
    """K of the host-side ``geometry()`` of csrc/superpixel.hip, read off the workspace size: for B = 16 the two per-centre
    arrays (48-byte centres, 16-byte boxes) take 16 * 64 * K bytes with no alignment padding, and the three per-pixel
    arrays (24 + 4 + 4 bytes) are rounded up to 256 bytes each."""
    from graphnet_classifier_amd import native
    total = native.load_library().gnc_slic_workspace_bytes(16, H, W, n_segments)
    assert total > 0

    def up(b):
        return (b + 255) // 256 * 256

    rest = total - up(16 * H * W * 24) - 2 * up(16 * H * W * 4)
    assert rest > 0 and rest % (16 * 64) == 0
    return rest // (16 * 64)


# ---------------------------------------------------------------------------------------------------------------- licence

@pytest.mark.parametrize("case", FIXTURES, ids=lambda c: f"case{c[0]}-{c[1].shape[0]}x{c[1].shape[1]}-{c[3]}")
def test_oracle_equals_scikit_image_on_every_fixture(case):
    _, img, ref, (n, c, mi, ec), _ = case
    labels, info = slic_oracle.slic(img, n_segments=n, compactness=c, max_iter=mi, enforce_connectivity=ec)
    assert labels.dtype == np.int32 and labels.shape == ref.shape
    mism = int((labels != ref).sum())
    assert mism == 0, f"{mism} of {ref.size} pixels differ"
    assert info["K"] == kernel_centre_count(img.shape[0], img.shape[1], n)
    if ec:
        assert info["n_labels"] == int(ref.max()) + 1 == len(np.unique(ref))
    else:
        assert info["n_labels"] == info["K"] and int(ref.max()) + 1 <= info["K"]


def test_fixture_seven_is_the_one_with_an_emptied_centre():
    emptied = [i for i, img, _, (n, c, mi, ec), _ in FIXTURES
               if slic_oracle.slic(img, n_segments=n, compactness=c, max_iter=mi, enforce_connectivity=False)[1]["emptied"]]
    assert emptied == [7]


def test_gamma_tables_of_kernel_and_oracle():
    """The kernel tabulates the 256 sRGB gamma values from the NumPy ``power`` that produced the fixtures; the oracle calls
    the ``power`` of the NumPy at hand.  NumPy's vectorised ``power`` is accurate to the last bit but not correctly rounded
    and differs between versions and CPUs there (the labels do not depend on it: the 44 fixtures).  So both are held to
    the C library's ``pow``, which Python's ``**`` calls and which is correctly rounded in all but rare cases: the linear
    part and both ends exactly, the rest within one unit in the last place."""
    with open(HIP) as f:
        src = f.read()
    body = src[src.index("kGamma[256] = {"):]
    body = body[:body.index("};")]
    table = np.array([float.fromhex(t) for t in re.findall(r"0x[0-9a-f.]+p[+-]\d+", body)])
    assert table.shape == (256,)
    v = [u * (1.0 / 255) for u in range(256)]
    libm = np.array([((x + 0.055) / 1.055) ** 2.4 if x > 0.04045 else x / 12.92 for x in v])
    for got in (table, slic_oracle.gamma_table()):
        assert np.array_equal(got[:11], libm[:11]) and got[255] == 1.0 and (np.diff(got) > 0).all()
        assert (np.abs(got - libm) <= np.spacing(libm)).all()


def test_connectivity_fill_by_hand():
    # a one-pixel island: below min_size 3 it takes the LAST labelled neighbour its fill met (right 1, then left / down / up 0)
    seg = np.array([[0, 0, 1], [0, 2, 1], [0, 0, 1]])
    out, n = slic_oracle.enforce_label_connectivity(seg, 3, 100, 0)
    assert n == 2 and out.dtype == np.int32 and np.array_equal(out, [[0, 0, 1], [0, 0, 1], [0, 0, 1]])
    # a fill capped at max_size 3: the rest of the run starts new labels; the last pixel alone is kept at min_size 0 ...
    row = np.zeros((1, 7), dtype=np.int64)
    out, n = slic_oracle.enforce_label_connectivity(row, 0, 3, 0)
    assert n == 3 and out.tolist() == [[0, 0, 0, 1, 1, 1, 2]]
    # ... and merged into its left neighbour at min_size 2
    out, n = slic_oracle.enforce_label_connectivity(row, 2, 3, 0)
    assert n == 2 and out.tolist() == [[0, 0, 0, 1, 1, 1, 1]]
    # start_label 1 (segments arrive shifted): same numbering plus one, and a component without any labelled neighbour is
    # set to 0, the value that means "not reached"
    out, n = slic_oracle.enforce_label_connectivity(row + 1, 2, 3, 1)
    assert n == 2 and out.tolist() == [[1, 1, 1, 2, 2, 2, 2]]
    out, n = slic_oracle.enforce_label_connectivity(np.ones((1, 1), dtype=np.int64), 2, 10, 1)
    assert n == 0 and out.tolist() == [[0]]


@pytest.mark.parametrize("shape,n,grid", [
    ((1, 128, 128), 100, ((0, 1), (6, 13), (6, 13))),      # square: both steps sqrt(16384 / 100) = 12.8
    ((1, 23, 200), 100, ((0, 1), (3, 7), (3, 7))),         # sqrt(4600 / 100) = 6.78 <= 23: still the square grid
    ((1, 7, 300), 100, ((0, 1), (2, 5), (2, 5))),          # sqrt(2100 / 100) = 4.58 <= 7: the same
    ((1, 7, 300), 12, ((0, 1), (3, 7), (12, 25))),         # sqrt(2100 / 12) = 13.2 > 7: one row, 300 / 12 apart
    ((1, 300, 7), 12, ((0, 1), (12, 25), (3, 7))),
    ((1, 120, 5), 6, ((0, 1), (10, 20), (2, 5))),
    ((1, 25, 25), 100, ((0, 1), (1, 2), (1, 2))),          # 2.5 rounds half to even
    ((1, 3, 130), 20, ((0, 1), (1, 3), (3, 6))),           # 130 / 20 = 6.5 as well
    ((1, 1, 40), 5, ((0, 1), (0, 1), (4, 8))),
    ((1, 40, 1), 7, ((0, 1), (2, 6), (0, 1))),             # 40 / 7 = 5.71: start 2, step 6
    ((1, 9, 7), 63, ((None, None),) * 3),                  # no more pixels than points: every pixel
    ((1, 9, 7), 62, ((0, 1), (0, 1), (0, 1))),             # sqrt(63 / 62) rounds to 1
])
def test_regular_grid_by_hand(shape, n, grid):
    got = slic_oracle.regular_grid(shape, n)
    assert tuple((s.start, s.step) for s in got) == grid


# ------------------------------------------------------------------------------------------------------------------ table

NAMES = [c[0] for c in S.CASES]


def _conn(kw):
    return kw.get("enforce_connectivity", True)


def test_table_size_and_budget():
    assert 60 <= len(S.CASES) <= 90
    for name, img, kw in S.CASES:
        H, W, n = S.row_of(name)
        assert img.dtype == np.uint8 and img.shape == (H, W, 3) and kw["n_segments"] == n
        assert H * W <= 190 * 250  # the connectivity scan is one lane per image
        if S.kind_of(name) == "noise":
            assert not _conn(kw)  # with connectivity it collapses to one label and tests nothing
    assert np.array_equal(S.CASES[0][1], S.KINDS["blobs"]("15x15-n9-blobs", 15, 15, 9))  # deterministic


def test_table_crosses_the_options():
    kws = [kw for _, _, kw in S.CASES]
    assert {0.5, 10.0, 30.0} <= {float(kw.get("compactness", 10.0)) for kw in kws}
    assert {1, 2, 10} <= {kw.get("max_iter", 10) for kw in kws}
    assert {(ec, sl) for ec in (True, False) for sl in (0, 1)} == {(_conn(kw), kw.get("start_label", 0)) for kw in kws}
    assert sum(kw.get("min_size_factor") == 0.0 for kw in kws) == 1 and sum(kw.get("max_size_factor") == 1.0 for kw in kws) == 1
    assert set(S.KINDS) == {S.kind_of(n) for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_case_meets_the_tables_conditions(name):
    _, img, kw = S.BY_NAME[name]
    labels, info = S.oracle(name)
    H, W, n = S.row_of(name)
    start = kw.get("start_label", 0)
    assert info["emptied"] == S.declared_emptied(name), "the case's id must say whether a centre was emptied"
    assert info["K"] == kernel_centre_count(H, W, n)
    assert labels.min() >= (0 if _conn(kw) else start)
    if _conn(kw):
        assert len(np.unique(labels[labels >= start])) == info["n_labels"]
        if S.kind_of(name) in ("blobs", "poster", "extremes") and min(H, W) >= 15:
            assert info["n_labels"] >= max(2, info["K"] // 3), "connectivity collapsed the case: retune the generator"
    else:
        assert info["n_labels"] == info["K"] and labels.max() < start + info["K"]


def test_every_shape_row_has_cases_without_an_emptied_centre():
    full = [n for n in NAMES if not S.oracle(n)[1]["emptied"]]
    assert len(full) >= 25
    rows = {S.row_of(n) for n in full}
    assert set(S.SHAPE_ROWS) - rows <= {S.ROW_WITHOUT_A_FULL_CASE}
    assert any(S.oracle(n)[1]["emptied"] for n in NAMES if S.row_of(n) == (100, 100, 1000))


def test_rows_reach_what_they_are_there_for():
    def steps(H, W, n):
        return slic_oracle._steps(slic_oracle.regular_grid((1, H, W), n))

    for H, W, n in S.SHAPE_ROWS:
        if (H, W, n) not in ((9, 7, 63), (9, 7, 100), (6, 5, 30)):
            assert H % 16 or W % 16  # a partly filled tile
    for H, W, n in ((23, 200, 100), (7, 300, 100)):  # thin, but the short side still holds the square step
        assert min(H, W) >= (H * W / n) ** 0.5 and steps(H, W, n)[1] == steps(H, W, n)[2] < min(H, W)
    for H, W, n in ((7, 300, 12), (120, 5, 6), (1, 40, 5), (40, 1, 7)):  # short side below the square step: the fallback branch
        assert min(H, W) < (H * W / n) ** 0.5 and min(steps(H, W, n)[1:]) == min(H, W) and (H, W, n) in S.SHAPE_ROWS
    for H, W, n in ((9, 7, 63), (9, 7, 100), (6, 5, 30)):
        assert steps(H, W, n) == [1, 1, 1]
        assert all(S.oracle(m)[1]["K"] == H * W for m in NAMES if S.row_of(m) == (H, W, n))  # every pixel a centre
    assert kernel_centre_count(100, 100, 1000) == 1089 > 4 * 256  # five candidate chunks in slic_assign
    # 190 x 250 (12): centres whose pixels span more than one 64-lane wave of slic_update (labels without connectivity
    # enforcement are the centre indices)
    near, _ = S.oracle("190x250-n12-blobs-conn0-start1")
    widths = [np.ptp(np.nonzero(near == k)[1]) + 1 for k in np.unique(near)]
    assert max(widths) > 2 * 64  # (the uniform image's boxes are 63 wide: the grid step)
    # the capped fill and the uncapped one, at partial-tile shapes
    _, capped = S.oracle("50x75-n100-blobs-max1")
    assert capped["n_labels"] > capped["K"]
    assert S.oracle("33x48-n100-blobs-min0")[1]["n_labels"] > S.oracle("33x48-n100-blobs")[1]["n_labels"]


def test_start_label_one_is_not_plus_one_under_connectivity():
    """why the GPU test compares start_label = 1 with the oracle and not with start_label = 0 plus one: a small component
    with no labelled neighbour is relabelled 0 either way"""
    differ = []
    for name in S.START_LABEL_CASES:
        _, _, kw = S.BY_NAME[name]
        assert _conn(kw) and kw.get("start_label", 0) == 0
        zero, _ = S.oracle(name)
        one, _ = S.oracle_at(name, **dict(kw, start_label=1))
        differ.append(not np.array_equal(one, zero + 1))
    assert any(differ)


def test_graph_cases_are_default_option_cases_without_emptied_centres():
    from graphnet_classifier_amd.image_to_graph import superpixel_capacities
    assert len(S.GRAPH_CASES) >= 6
    for name in S.GRAPH_CASES:
        _, img, kw = S.BY_NAME[name]
        H, W, _ = S.row_of(name)
        assert set(kw) <= {"n_segments", "compactness"} and not S.declared_emptied(name) and (H % 16 or W % 16)
        # the graph fits the capacities the batched build derives from n_segments: its overflow flag must stay 0
        x, _, ei = IO.superpixel_graph_from_labels(img, S.oracle(name)[0])
        nodes, edges = superpixel_capacities(kw["n_segments"])
        assert x.shape[0] == S.oracle(name)[1]["n_labels"] <= nodes and ei.shape[1] <= edges
    for shape, names in S.BATCH_CASES.items():
        assert len(names) == 5 and len({S.BY_NAME[n][1].tobytes() for n in names}) == 5
        assert all(S.BY_NAME[n][1].shape[:2] == shape for n in names)
