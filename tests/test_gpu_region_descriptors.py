"""GPU: the region descriptor kernel (csrc/region_descriptor.hip, DESIGN K26) against the NumPy reference of
tests/region_descriptor_reference.py: whole output buffers - padding rows and counts included - bit for bit, on the superpixel
fixtures (in batches and alone) and on synthetic label images that each aim at one accumulator or branch.

The five columns behind a double-precision ``sqrt`` (3-5, 9, 10) are held to bit equality like the others: the device
``sqrt`` is correctly rounded, as the reference's is."""
import collections

import numpy as np
import pytest
import torch

from tests import region_descriptor_reference as R
from tests.test_superpixel_golden import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def I2G():
    from graphnet_classifier_amd import image_to_graph
    return image_to_graph


def _run(I2G, imgs, labs, cap=512):
    desc, counts = I2G.region_descriptors(np.ascontiguousarray(imgs), np.ascontiguousarray(labs), node_capacity=cap)
    assert desc.is_cuda and desc.dtype == torch.float32 and counts.dtype == torch.int32
    assert tuple(desc.shape) == (len(imgs), cap, 16) and tuple(counts.shape) == (len(imgs), 3)
    return desc.cpu().numpy(), counts.cpu().numpy()


def _assert_bits(got, want, what=""):
    """float32 buffers equal bit for bit; on a mismatch, say which columns differ and by how many ulps"""
    g, w = np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32)
    if np.array_equal(g, w):
        return
    diff = np.abs(g.astype(np.int64) - w.astype(np.int64))
    cols = sorted(set(np.argwhere(diff)[:, -1].tolist()))
    raise AssertionError(f"{what}: {int((diff != 0).sum())} entries differ, in columns {cols}, by at most {int(diff.max())} float32 ulps")


def _check(I2G, imgs, labs, cap=512, what=""):
    """kernel == reference over the whole buffers; returns the kernel's (desc, counts)"""
    desc, counts = _run(I2G, imgs, labs, cap)
    want, want_counts = R.region_descriptors_batch(imgs, labs, cap)
    assert np.array_equal(counts, want_counts), (what, counts.tolist(), want_counts.tolist())
    _assert_bits(desc, want, what)
    return desc, counts


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (3,), dtype=np.uint8)


def _by_size():
    groups = collections.OrderedDict()
    for c in CASES:
        groups.setdefault(c[1].shape[:2], []).append(c)
    return groups


@pytest.fixture(scope="module")
def fixture_batches(I2G):
    """(cases, kernel desc, kernel counts) per image size: all cases of 32 x 32, 64 x 64 and 96 x 160, one of 128 x 128 and 256 x 256"""
    out = {}
    for shape, cases in _by_size().items():
        if shape in ((128, 128), (256, 256)):
            cases = cases[:1]
        imgs, labs = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
        out[shape] = (cases, imgs, labs) + _check(I2G, imgs, labs, what=f"fixtures {shape}")
    return out


def test_fixture_cases_in_batches(fixture_batches):
    assert {(32, 32), (64, 64), (96, 160), (128, 128), (256, 256)} <= set(fixture_batches)
    for shape, (cases, _, _, desc, counts) in fixture_batches.items():
        assert not counts[:, 1:].any()
        for b, c in enumerate(cases):
            if c[4] is not None:  # the reference's own graph: its x is columns 0-2
                assert counts[b, 0] == len(c[4][0]) and np.array_equal(desc[b, :counts[b, 0], :3], c[4][0])
        assert desc.min() >= 0.0 and desc.max() <= 1.0


def test_every_case_alone_has_the_bits_of_its_batch(I2G, fixture_batches):
    for shape, (cases, imgs, labs, desc, counts) in fixture_batches.items():
        for b in range(len(cases)):
            alone, alone_counts = _run(I2G, imgs[b:b + 1], labs[b:b + 1])
            assert np.array_equal(alone_counts[0], counts[b])
            _assert_bits(alone[0], desc[b], f"{shape} case {b} alone")


def test_single_image_form_reads_its_count(I2G, fixture_batches):
    cases, imgs, labs, desc, counts = fixture_batches[(32, 32)]
    one, c = I2G.region_descriptors(imgs[0], labs[0])
    assert tuple(one.shape) == (counts[0, 0], 16) and c.tolist() == counts[0].tolist()
    _assert_bits(one.cpu().numpy(), desc[0, :counts[0, 0]], "single image")
    with pytest.raises(NotImplementedError, match="512"):
        I2G.region_descriptors(imgs[0], labs[0], node_capacity=4)
    bad = labs[0].copy()
    bad[3, 3] = -1
    with pytest.raises(ValueError, match="outside"):
        I2G.region_descriptors(imgs[0], bad)


def test_region_counts_equal_the_region_graph_build(I2G, fixture_batches):
    for shape, (cases, imgs, labs, desc, counts) in fixture_batches.items():
        batch = I2G.superpixel_graphs_batched(imgs, labs, node_capacity=512, edge_capacity=4096)
        assert batch.counts[:, 0].tolist() == counts[:, 0].tolist()
        n = counts[:, 0]
        for b in range(len(cases)):  # and row i is node i: the mean colour is the build's x
            assert np.array_equal(batch.x[b, :n[b]].cpu().numpy(), desc[b, :n[b], :3])


def test_labels_with_gaps_and_in_descending_order(I2G, fixture_batches):
    cases, imgs, labs, desc, counts = fixture_batches[(64, 64)]
    gaps, _ = _check(I2G, imgs[:3], 7 * labs[:3] + 11, what="gaps")
    _assert_bits(gaps, desc[:3], "labels with gaps")
    flipped = labs[:3].max() - labs[:3]  # label order against the raster order: the rows come out reversed
    rev, rc = _check(I2G, imgs[:3], flipped, what="descending")
    for b in range(3):
        n = counts[b, 0]
        if labs[b].max() == n - 1 and labs[:3].max() == labs[b].max():
            _assert_bits(rev[b, :n], desc[b, :n][::-1], "descending labels")


def _sliver_labels():
    lab = np.zeros((16, 24), np.int32)
    lab[5, 7] = 4               # a single pixel: m = 0, both stds 0, box fill 1
    lab[2, 3:20] = 9            # 1 x 17
    lab[1:15, 22] = 2           # 14 x 1
    lab[8:12, 1:3] = 30         # a 4 x 2 block
    return lab


def test_single_pixel_and_sliver_regions(I2G):
    lab = _sliver_labels()
    img = _noise(lab.shape, 1)
    desc, counts = _check(I2G, img[None], lab[None], cap=8, what="slivers")
    assert counts[0].tolist() == [5, 0, 0]
    single = desc[0, 2]  # labels 0, 2, 4, 9, 30 -> rows 0 .. 4
    assert not single[3:6].any() and not single[9:11].any() and not single[13:].any() and single[11] == 1.0 and single[12] == 1.0
    row, column = desc[0, 3], desc[0, 1]
    assert row[7] == np.float32(1 / 16) and row[8] == np.float32(17 / 24) and row[9] == 0.0 and row[11] == 1.0 and row[12] == 1.0
    assert column[7] == np.float32(14 / 16) and column[8] == np.float32(1 / 24) and column[10] == 0.0 and column[11] == 1.0


def test_checkerboard_of_single_pixel_regions(I2G):
    lab = np.arange(256, dtype=np.int32).reshape(16, 16)
    img = _noise(lab.shape, 2)
    desc, counts = _check(I2G, img[None], lab[None], cap=256, what="pixel regions")
    assert counts[0].tolist() == [256, 0, 0]
    assert (desc[0, :, 12] == 1.0).all() and not desc[0, :, 13:].any() and (desc[0, :, 6] == np.float32(1 / 256)).all()
    assert np.array_equal(desc[0, :, :3], (img.reshape(-1, 3) / 255.0).astype(np.float32))


def test_one_region_covering_the_image(I2G):
    img = _noise((40, 56), 3)
    desc, counts = _check(I2G, img[None], np.full((1, 40, 56), 5, np.int32), cap=2, what="one region")
    assert counts[0].tolist() == [1, 0, 0]
    assert desc[0, 0, 6] == 1.0 and desc[0, 0, 7] == 1.0 and desc[0, 0, 8] == 1.0 and desc[0, 0, 11] == 1.0 and desc[0, 0, 12] == 0.0


def test_largest_square_sums_and_largest_texture(I2G):
    white = np.full((256, 256, 3), 255, np.uint8)  # Q_c = 65025 * 65536 = 4,261,478,400, just under 2^32
    yy, xx = np.mgrid[:256, :256]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)  # every pair differs by 255: largest T_c
    labs = np.zeros((2, 256, 256), np.int32)
    desc, counts = _check(I2G, np.stack([white, board]), labs, cap=4, what="256 x 256 extremes")
    assert counts.tolist() == [[1, 0, 0]] * 2
    assert desc[0, 0, :3].tolist() == [1.0] * 3 and not desc[0, 0, 3:6].any() and not desc[0, 0, 13:].any()
    assert desc[1, 0, 13:].tolist() == [1.0] * 3 and desc[1, 0, :3].tolist() == [0.5] * 3 and desc[1, 0, 3:6].tolist() == [0.5] * 3


@pytest.mark.parametrize("shape", [(1, 65536), (65536, 1)], ids=["row", "column"])
def test_longest_line_images(I2G, shape):
    """the 64-bit second moments (n Syy passes 2^53) and no vertical / horizontal pairs at all"""
    img = _noise(shape, 4)
    one = np.zeros(shape, np.int32)
    two = one.copy()
    two.reshape(-1)[40000:] = 3
    desc, counts = _check(I2G, np.stack([img, img]), np.stack([one, two]), cap=4, what=f"line {shape}")
    assert counts.tolist() == [[1, 0, 0], [2, 0, 0]]
    spread, flat = (10, 9) if shape[0] == 1 else (9, 10)
    assert desc[0, 0, flat] == 0.0 and abs(float(desc[0, 0, spread]) - 12 ** -0.5) < 1e-6
    assert desc[1, 0, 12] == np.float32(1 / 40000) and desc[1, 1, 12] == np.float32(1 / 25536)


def _pairs_32(count):
    """a 32 x 32 label image with `count` regions: 2-pixel regions, the last ones split into single pixels"""
    lab = (np.arange(1024, dtype=np.int32) // 2).reshape(32, 32)
    extra = count - 512
    flat = lab.reshape(-1)
    for k in range(extra):
        flat[2 * k + 1] = 600 + k
    return lab


def test_exactly_512_regions(I2G):
    lab = _pairs_32(512)
    desc, counts = _check(I2G, _noise((32, 32), 5)[None], lab[None], what="512 regions")
    assert counts[0].tolist() == [512, 0, 0] and (desc[0, :, 6] == np.float32(2 / 1024)).all()


def test_overflow_flags_its_own_image_only(I2G):
    imgs = np.stack([_noise((32, 32), 6 + k) for k in range(3)])
    labs = np.stack([_pairs_32(512), _pairs_32(513), _pairs_32(512)[::-1].copy()])
    desc, counts = _check(I2G, imgs, labs, what="513 regions")
    assert counts.tolist() == [[512, 0, 0], [513, 0, 1], [512, 0, 0]] and not desc[1].any() and desc[0].any() and desc[2].any()
    lab4 = (np.arange(1024, dtype=np.int32) // 4).reshape(32, 32)  # 256 regions
    desc, counts = _check(I2G, imgs, np.stack([lab4 // 2, lab4, lab4 // 4]), cap=128, what="capacity below the count")
    assert counts.tolist() == [[128, 0, 0], [256, 0, 1], [64, 0, 0]] and not desc[1].any() and not desc[2, 64:].any()


def test_bad_labels_flag_their_own_image_only(I2G, fixture_batches):
    cases, imgs, labs, good, _ = fixture_batches[(64, 64)]
    labs = labs[:3].copy()
    labs[1, 10, 10] = -1
    labs[1, 63, 63] = 64 * 64
    desc, counts = _check(I2G, imgs[:3], labs, what="bad labels")
    assert counts[:, 1].tolist() == [0, 1, 0] and not desc[1].any()
    _assert_bits(desc[0], good[0], "neighbour of a bad image")
    _assert_bits(desc[2], good[2], "neighbour of a bad image")


@pytest.mark.parametrize("shape", [(33, 31), (5, 7), (41, 100), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_runs_that_end_mid_region_and_mid_row(I2G, shape):
    """sizes that are no multiple of the 1024 threads: a thread's run of consecutive pixels starts and ends inside a row and inside
    a region (33 x 31 = 1023 pixels: one per thread, one thread idle; 41 x 100: runs of 5 over rows of 100 and blocks of 6 x 9)"""
    H, W = shape
    yy, xx = np.mgrid[:H, :W]
    lab = ((yy // 6) * 40 + xx // 9).astype(np.int32)
    img = _noise(shape, 9)
    _check(I2G, np.stack([img, img[::-1, ::-1]]), np.stack([lab, lab]), cap=128, what=f"blocks {shape}")


def test_buffers_behind_the_outputs_stay_untouched(I2G):
    from graphnet_classifier_amd import native
    lib = native.load_library()
    dev = torch.device("cuda")
    cases = [c for c in CASES if c[1].shape[:2] == (32, 32)][:2]
    imgs = torch.from_numpy(np.stack([c[1] for c in cases])).to(dev)
    labs = torch.from_numpy(np.stack([c[2] for c in cases])).to(dev)
    B, cap = 2, 48
    out = torch.full((B + 1, cap, 16), 7.0, device=dev)
    counts = torch.full((B + 1, 3), 7, dtype=torch.int32, device=dev)
    nbytes = lib.gnc_region_descriptors_workspace_bytes(B, 32, 32, cap)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    native._check(lib.gnc_region_descriptors_rgb_u8(labs.data_ptr(), imgs.data_ptr(), B, 32, 32, cap, out.data_ptr(), counts.data_ptr(),
                                                    ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "descriptors")
    torch.cuda.synchronize()
    assert bool((out[B] == 7).all()) and bool((counts[B] == 7).all())
    want, want_counts = R.region_descriptors_batch([c[1] for c in cases], [c[2] for c in cases], cap)
    assert np.array_equal(counts[:B].cpu().numpy(), want_counts)
    _assert_bits(out[:B].cpu().numpy(), want, "guarded buffers")
