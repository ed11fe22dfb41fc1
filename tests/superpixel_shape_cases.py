"""Case table of the device SLIC at shapes the fixtures do not reach, shared by tests/test_slic_oracle_host.py and
tests/test_gpu_superpixel_shapes.py.  No GPU here.

Every fixture image of tests/golden/g10_superpixel*.npz has sides that are multiples of 16, the tile of ``slic_assign``
(csrc/superpixel.hip).  The shapes below are the smallest that reach what those cannot: partly filled tiles, centre boxes
with ragged right edges, the short-side branch of ``regular_grid``, unit steps, several 256-candidate chunks, boxes wider
than a wave.  The reference is the sequential NumPy SLIC of oracle/slic_oracle.py, which tests/test_slic_oracle_host.py
pins to all 44 fixtures.

A case is ``(name, image uint8 [H, W, 3], slic kwargs)``; images come from a generator seeded by the case's name.  A name
that ends in ``-emptied`` declares that some centre loses all its pixels on the way (the oracle's ``info["emptied"]``;
the host test holds the declaration to the oracle): those lean on the empty-centre rule that only fixture 7 pins.
"""
import functools
import zlib

import numpy as np

from oracle import slic_oracle

# ------------------------------------------------------------------------------------------------------------------ images


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def _field(rng, H, W, n_segments):
    """float [H, W, 3] in about [0, 1]: per channel a few cosines whose wavelengths are 3 - 8 seed-grid steps."""
    step = max(2.0, (H * W / max(1, min(n_segments, H * W))) ** 0.5)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(4):
            wave = step * rng.uniform(3.0, 8.0)
            ang = rng.uniform(0.0, 2.0 * np.pi)
            out[..., c] += np.cos(2.0 * np.pi * (yy * np.cos(ang) + xx * np.sin(ang)) / wave + rng.uniform(0.0, 2.0 * np.pi))
    return 0.5 + out / 8.0 * 1.6


def blobs(name, H, W, n_segments):
    """smooth low-frequency colour fields plus mild noise (two grey levels)"""
    rng = _rng(name)
    v = _field(rng, H, W, n_segments) * 255.0 + rng.uniform(-2.0, 2.0, size=(H, W, 3))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def poster(name, H, W, n_segments):
    """a blobs image quantised to 4 levels per channel: flat regions, so exact distance ties are common"""
    q = blobs(name, H, W, n_segments) // 64
    return (q * 85).astype(np.uint8)


def noise(name, H, W, n_segments):
    return _rng(name).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def uniform(name, H, W, n_segments):
    return np.full((H, W, 3), _rng(name).integers(0, 256, size=3, dtype=np.uint8), dtype=np.uint8)


def extremes(name, H, W, n_segments):
    """patches of the 8 corners of the colour cube (pure primaries, black, white): both ends of the gamma table and
    both sides of the 0.008856 cube-root switch of xyz2lab"""
    rng = _rng(name)
    step = max(2, int(round((H * W / max(1, min(n_segments, H * W))) ** 0.5 * 1.7)))
    gh, gw = -(-H // step) + 1, -(-W // step) + 1
    corners = rng.integers(0, 2, size=(gh, gw, 3), dtype=np.uint8) * 255
    oy, ox = int(rng.integers(0, step)), int(rng.integers(0, step))
    return np.ascontiguousarray(np.repeat(np.repeat(corners, step, axis=0), step, axis=1)[oy:oy + H, ox:ox + W])


KINDS = dict(blobs=blobs, poster=poster, noise=noise, uniform=uniform, extremes=extremes)

# ------------------------------------------------------------------------------------------------------------------- table

OFF = dict(enforce_connectivity=False)

# (H, W, n_segments) -> [(kind, slic options, declared emptied)]
TABLE = {
    # one partly filled tile
    (15, 15, 9): [("blobs", {}, False), ("poster", {}, True), ("uniform", dict(start_label=1), False),
                  ("noise", OFF, False), ("extremes", dict(max_iter=2), True)],
    # one column in a second tile
    (16, 17, 12): [("blobs", {}, False), ("poster", dict(compactness=30.0), False), ("uniform", OFF, False),
                   ("extremes", dict(start_label=1), True)],
    # partial tiles on one or both edges, H > W and H < W
    (17, 23, 10): [("blobs", {}, False), ("poster", dict(max_iter=1), False), ("noise", dict(OFF, start_label=1), False),
                   ("extremes", {}, True)],
    (31, 47, 100): [("blobs", {}, False), ("poster", {}, True), ("uniform", {}, False),
                    ("blobs", dict(OFF, compactness=0.5), False), ("extremes", dict(compactness=30.0), True)],
    (33, 48, 100): [("blobs", {}, False), ("poster", dict(start_label=1), True), ("extremes", {}, True),
                    ("noise", OFF, True), ("blobs", dict(min_size_factor=0.0), False),
                    ("uniform", dict(max_iter=2), False)],
    (50, 75, 100): [("blobs", {}, False), ("poster", {}, True), ("extremes", dict(OFF), True),
                    ("blobs", dict(max_size_factor=1.0), False), ("blobs", dict(compactness=30.0, start_label=1), False),
                    ("noise", dict(OFF, max_iter=2), False)],
    (100, 100, 100): [("blobs", {}, False), ("poster", {}, True), ("extremes", {}, True), ("uniform", {}, False),
                      ("blobs", dict(compactness=0.5), False), ("noise", dict(OFF, compactness=30.0), False)],
    (129, 65, 100): [("blobs", {}, False), ("poster", dict(OFF), True), ("extremes", dict(max_iter=1), False),
                     ("blobs", dict(start_label=1, max_iter=2), False), ("uniform", dict(OFF), False)],
    # thin images (at 100 segments the short side still holds the square step: regular_grid's first branch)
    (23, 200, 100): [("blobs", {}, False), ("poster", {}, True), ("extremes", {}, True), ("noise", OFF, False),
                     ("uniform", dict(start_label=1), False)],
    (7, 300, 100): [("blobs", {}, False), ("poster", dict(compactness=30.0), False), ("uniform", {}, False),
                    ("noise", OFF, False)],
    # short side below the square step: the fallback branch of regular_grid, one row / one column of seeds
    (7, 300, 12): [("blobs", {}, False), ("poster", dict(OFF), False), ("uniform", dict(start_label=1), False)],
    (120, 5, 6): [("blobs", {}, False), ("poster", {}, False), ("uniform", dict(OFF), False)],
    # steps that end in .5 and round half to even: sqrt(625 / 100) = 2.5 -> 2, 130 / 20 = 6.5 -> 6
    (25, 25, 100): [("blobs", {}, False), ("uniform", dict(OFF), False)],
    (3, 130, 20): [("blobs", {}, False), ("uniform", dict(OFF), False)],
    # one-pixel dimensions (the fallback branch again)
    (1, 40, 5): [("blobs", {}, False), ("uniform", dict(start_label=1), False), ("noise", OFF, False)],
    (40, 1, 7): [("blobs", {}, False), ("poster", dict(OFF), False), ("uniform", {}, False)],
    # H * W <= n_segments: unit steps
    (9, 7, 63): [("blobs", {}, False), ("uniform", {}, False), ("noise", OFF, False)],
    (9, 7, 100): [("blobs", dict(start_label=1), False), ("poster", dict(OFF), False), ("uniform", dict(max_iter=1), False)],
    (6, 5, 30): [("blobs", {}, False), ("uniform", dict(OFF, start_label=1), False), ("extremes", {}, False)],
    # K = 1089: several 256-candidate chunks at a partial-tile size, many emptied centres
    (100, 100, 1000): [("blobs", {}, False), ("poster", dict(OFF), True), ("noise", OFF, True),
                       ("uniform", {}, False), ("blobs", dict(compactness=30.0, max_iter=2), False)],
    # centre boxes wider than one 64-lane wave
    (190, 250, 12): [("blobs", {}, False), ("poster", {}, False), ("extremes", dict(compactness=30.0), True),
                     ("uniform", dict(OFF), False), ("blobs", dict(OFF, start_label=1), False)],
}

SHAPE_ROWS = tuple(TABLE)
ROW_WITHOUT_A_FULL_CASE = (100, 100, 1000)  # the one row that may consist of emptied cases only


def _opts_id(kw):
    short = dict(compactness="c", max_iter="it", enforce_connectivity="conn", start_label="start", min_size_factor="min",
                 max_size_factor="max")
    return "".join(f"-{short[k]}{int(v) if isinstance(v, bool) else v:g}" for k, v in kw.items())


def _build():
    cases, rows = [], {}
    for (H, W, n), entries in TABLE.items():
        for kind, kw, emptied in entries:
            name = f"{H}x{W}-n{n}-{kind}{_opts_id(kw)}" + ("-emptied" if emptied else "")
            img = KINDS[kind](name.removesuffix("-emptied"), H, W, n)
            cases.append((name, img, dict(kw, n_segments=n)))
            rows[name] = ((H, W, n), kind)
    assert len({c[0] for c in cases}) == len(cases)
    return cases, rows


CASES, _ROWS = _build()
BY_NAME = {c[0]: c for c in CASES}


# connectivity on, start_label 0 in the table: run again at start_label = 1 against the oracle at start_label = 1.  In the
# first a one-pixel leftover keeps the value 0, in the second 120 pixels are numbered differently: a small component whose
# fill met no labelled neighbour is set to 0, which under start_label = 1 means "not reached yet", so the scan seeds its
# remaining pixels again.
START_LABEL_CASES = ("16x17-n12-blobs", "100x100-n100-blobs-c0.5", "33x48-n100-blobs-min0", "50x75-n100-blobs-max1",
                     "129x65-n100-blobs", "23x200-n100-poster-emptied", "7x300-n100-blobs", "40x1-n7-blobs")

# default options, partial tiles, no emptied centre: the region graph downstream of the labels
GRAPH_CASES = ("15x15-n9-blobs", "17x23-n10-blobs", "31x47-n100-blobs", "33x48-n100-blobs", "50x75-n100-blobs",
               "129x65-n100-blobs", "23x200-n100-blobs")

# five different images of one partial-tile shape for a batched call (at the default options, not the cases' own)
BATCH_CASES = {
    (33, 48): ("33x48-n100-blobs", "33x48-n100-poster-start1-emptied", "33x48-n100-extremes-emptied",
               "33x48-n100-blobs-min0", "33x48-n100-noise-conn0-emptied"),
    (50, 75): ("50x75-n100-blobs", "50x75-n100-poster-emptied", "50x75-n100-extremes-conn0-emptied",
               "50x75-n100-blobs-max1", "50x75-n100-blobs-c30-start1"),
}
BATCH_ORACLE_IMAGE = 3  # "image 3 of the batch equals the oracle": a blobs image in both


def row_of(name):
    """(H, W, n_segments) of the shape-table row the case belongs to"""
    return _ROWS[name][0]


def kind_of(name):
    return _ROWS[name][1]


def declared_emptied(name) -> bool:
    return name.endswith("-emptied")


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(labels int32 [H, W], info) of the sequential oracle for the case, computed once per process and read-only"""
    _, img, kw = BY_NAME[name]
    labels, info = slic_oracle.slic(img, **kw)
    labels.setflags(write=False)
    return labels, info


@functools.lru_cache(maxsize=None)
def _oracle_at(name, items):
    labels, info = slic_oracle.slic(BY_NAME[name][1], **dict(items))
    labels.setflags(write=False)
    return labels, info


def oracle_at(name, **kw):
    """the oracle for the case's image at exactly the options ``kw`` (not the case's own)"""
    return _oracle_at(name, tuple(sorted(kw.items())))
