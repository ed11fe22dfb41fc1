"""GPU: the device augmentation (csrc/augment.hip, K25) against live Pillow, byte for byte: ``crop_resize`` against
``crop().resize().transpose()``, ``color_jitter`` against chains of ``ImageEnhance``, and the folder loaders against the graphs
and tensors of the images Pillow produces from the same sampled parameters."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from graphnet_classifier_amd import dataset as D
from graphnet_classifier_amd import image_to_graph as I2G
from graphnet_classifier_amd import native
from graphnet_classifier_amd.augment import Augmentation
from tests import augment_reference as R

pytestmark = pytest.mark.gpu

FILTERS = ["bicubic", "bilinear", "box"]

# (image (H, W), box (left, top, right, bottom), output (W, H)): what each case is there for
CROP_CASES = [
    ((37, 53), (0, 0, 53, 37), (20, 24)),     # the whole image
    ((37, 53), (17, 9, 18, 10), (1, 1)),      # 1 x 1 boxes
    ((37, 53), (17, 9, 18, 10), (7, 5)),
    ((37, 53), (0, 0, 1, 1), (4, 3)),
    ((37, 53), (52, 36, 53, 37), (3, 4)),
    ((37, 53), (20, 0, 21, 37), (6, 9)),      # one column
    ((37, 53), (20, 3, 21, 30), (1, 50)),
    ((37, 53), (0, 11, 53, 12), (16, 5)),     # one row
    ((37, 53), (4, 11, 47, 12), (90, 1)),
    ((37, 53), (0, 5, 30, 20), (16, 16)),     # touching the left, top, right and bottom borders
    ((37, 53), (5, 0, 30, 20), (16, 16)),
    ((37, 53), (25, 5, 53, 20), (16, 16)),
    ((37, 53), (5, 20, 30, 37), (16, 16)),
    ((41, 67), (1, 2, 40, 30), (24, 20)),     # left = 1, 2, 3 on odd widths: a row starts on every byte alignment
    ((41, 67), (2, 2, 40, 30), (24, 20)),
    ((41, 67), (3, 2, 40, 30), (24, 20)),
    ((40, 35), (1, 0, 34, 40), (50, 40)),     # ... with the height unchanged, so the horizontal pass stores the output
    ((40, 35), (2, 0, 34, 40), (11, 40)),
    ((40, 35), (3, 0, 34, 40), (64, 40)),
    ((64, 48), (3, 1, 40, 2), (16, 8)),       # top and box heights that are no multiples of 4
    ((64, 48), (3, 3, 40, 6), (16, 8)),
    ((64, 48), (3, 5, 40, 10), (16, 2)),
    ((64, 48), (3, 7, 40, 14), (16, 30)),
    ((64, 48), (5, 3, 44, 64), (39, 20)),     # the width unchanged: the vertical pass reads the source at the image's pitch
    ((97, 131), (10, 20, 30, 40), (128, 128)),  # up- and down-scaling
    ((375, 500), (33, 41, 470, 340), (128, 128)),
    ((375, 500), (100, 50, 228, 178), (128, 128)),  # the box has the output's size: the copy path
    ((37, 53), (7, 3, 27, 19), (20, 16)),
    ((37, 53), (7, 3, 27, 19), (1, 16)),      # out_w = 1
    ((37, 53), (7, 3, 27, 19), (13, 16)),     # an odd and an even out_w under a flip
    ((37, 53), (7, 3, 27, 19), (14, 9)),
    ((2, 11010), (5, 1, 11005, 2), (300, 1)),  # a 1 x 11000 box: rows beyond the staging limit are read where they lie
    ((2, 11010), (3, 0, 11003, 2), (50, 3)),
    ((3, 10950), (7, 0, 10929, 3), (40, 2)),   # ... and the longest row that is still staged (10922 pixels)
]


def _mismatch(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    return int((got != want).sum())


@pytest.fixture(scope="module")
def crop_sources():
    return {hw: R.rand_img(*hw) for hw in {c[0] for c in CROP_CASES}}


@pytest.mark.parametrize("name", FILTERS)
def test_crop_resize_equals_pillow(crop_sources, name):
    bad = []
    for hw, box, size in CROP_CASES:
        img = crop_sources[hw]
        for flip in (False, True):
            got = I2G.crop_resize(img, box, size, name, None if not flip else [True])
            assert got.is_cuda and got.dtype == torch.uint8
            mism = _mismatch(got, R.pil_crop_resize(img, box, size, name, flip))
            if mism:
                bad.append((hw, box, size, flip, mism))
    assert not bad, bad


@pytest.mark.parametrize("name", FILTERS)
def test_whole_image_box_equals_resize(name):
    for hw, size in [((37, 53), (20, 24)), ((37, 53), (53, 37)), ((97, 61), (128, 128))]:
        img = R.rand_img(*hw)
        got = I2G.crop_resize(img, (0, 0, hw[1], hw[0]), size, name)
        assert torch.equal(got, I2G.resize(img, size, name))


@pytest.mark.parametrize("name", ["bicubic", "box"])
def test_mixed_size_batch_equals_per_image(name):
    shapes = [(375, 500), (1, 1), (128, 128), (129, 300), (77, 13), (64, 200), (500, 375), (128, 57)]
    boxes = [(13, 7, 401, 300), (0, 0, 1, 1), (0, 0, 128, 128), (1, 2, 300, 129), (3, 9, 12, 70), (2, 0, 130, 64), (7, 0, 8, 375),
             (0, 100, 57, 101)]
    flips = [True, False, True, False, True, True, False, True]
    imgs = [R.rand_img(h, w, seed=k) for k, (h, w) in enumerate(shapes)]
    batch = I2G.crop_resize(imgs, np.array(boxes), (128, 96), name, np.array(flips))
    assert tuple(batch.shape) == (len(imgs), 96, 128, 3)
    for k, img in enumerate(imgs):
        assert torch.equal(batch[k], I2G.crop_resize(img, boxes[k], (128, 96), name, [flips[k]])), k
        assert _mismatch(batch[k], R.pil_crop_resize(img, boxes[k], (128, 96), name, flips[k])) == 0, k
    dev = I2G.crop_resize([torch.from_numpy(im).cuda() for im in imgs], boxes, (128, 96), name, flips)
    assert torch.equal(dev, batch)
    # a dense batch
    dense = np.stack([R.rand_img(60, 80, seed=k) for k in range(5)])
    dboxes = np.array([(0, 0, 80, 60), (1, 1, 79, 59), (30, 0, 31, 60), (3, 5, 67, 53), (2, 50, 80, 60)])
    dflips = np.array([False, True, True, False, True])
    for src in (dense, torch.from_numpy(dense).cuda(), list(dense)):
        out = I2G.crop_resize(src, dboxes, (64, 48), name, dflips)
        for k in range(5):
            assert _mismatch(out[k], R.pil_crop_resize(dense[k], dboxes[k], (64, 48), name, dflips[k])) == 0, k


def test_crop_resize_replays_under_graph_capture():
    imgs = np.stack([R.rand_img(200, 150, seed=k) for k in range(4)])
    boxes = np.array([(1, 2, 140, 190), (0, 0, 150, 200), (33, 17, 97, 81), (149, 0, 150, 200)])
    flips = np.array([True, False, False, True])
    src, dbox, dflip = torch.from_numpy(imgs).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(flips).cuda()
    eager = I2G.crop_resize(src, dbox, (64, 64), "bicubic", dflip)
    assert torch.equal(eager, I2G.crop_resize(imgs, boxes, (64, 64), "bicubic", flips))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        I2G.crop_resize(src, dbox, (64, 64), "bicubic", dflip)  # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = I2G.crop_resize(src, dbox, (64, 64), "bicubic", dflip)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    imgs2 = np.stack([R.rand_img(200, 150, seed=10 + k) for k in range(4)])
    boxes2 = np.array([(10, 20, 74, 84), (3, 0, 150, 199), (0, 199, 150, 200), (5, 6, 50, 60)])
    flips2 = np.array([False, True, True, False])
    src.copy_(torch.from_numpy(imgs2))
    dbox.copy_(torch.from_numpy(boxes2))
    dflip.copy_(torch.from_numpy(flips2))
    g.replay()
    torch.cuda.synchronize()
    for k in range(4):
        assert _mismatch(captured[k], R.pil_crop_resize(imgs2[k], boxes2[k], (64, 64), "bicubic", flips2[k])) == 0, k


def test_a_device_box_outside_its_image_is_skipped_not_read():
    src = torch.from_numpy(np.stack([R.rand_img(20, 30, seed=k) for k in range(3)])).cuda()
    boxes = torch.tensor([(0, 0, 31, 20), (2, 3, 20, 15), (5, 5, 5, 10)], dtype=torch.int64).cuda()
    lib = native.load_library()
    out = torch.full((3, 8, 8, 3), 99, dtype=torch.uint8, device="cuda")
    table = torch.cat([boxes, torch.zeros(3, 1, dtype=torch.int64, device="cuda")], dim=1).contiguous()
    nbytes = lib.gnc_crop_resize_workspace_bytes(3, 20, 30, 8, 8, 3)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    native._check(lib.gnc_crop_resize_rgb_u8(src.data_ptr(), None, table.data_ptr(), 3, 20, 30, 8, 8, 3, out.data_ptr(), ws.data_ptr(),
                                             nbytes, torch.cuda.current_stream().cuda_stream), "gnc_crop_resize_rgb_u8")
    assert (out[0] == 99).all() and (out[2] == 99).all()
    assert _mismatch(out[1], R.pil_crop_resize(src[1].cpu().numpy(), (2, 3, 20, 15), (8, 8))) == 0


def test_crop_resize_rejects_bad_input():
    img = R.rand_img(8, 10)
    for box in [(0, 0, 11, 8), (0, 0, 10, 9), (-1, 0, 5, 5), (0, -1, 5, 5), (5, 0, 5, 8), (6, 0, 5, 8), (0, 4, 10, 4), (0, 5, 10, 4)]:
        with pytest.raises(ValueError, match="empty or leaves"):
            I2G.crop_resize(img, box, (4, 4))
    with pytest.raises(ValueError):
        I2G.crop_resize([img, img], [(0, 0, 4, 4)], (4, 4))
    with pytest.raises(ValueError):
        I2G.crop_resize([img, img], [(0, 0, 4, 4)] * 2, (4, 4), flip=[True])
    with pytest.raises(ValueError):
        I2G.crop_resize(img, (0, 0, 4), (4, 4))
    with pytest.raises(ValueError):
        I2G.crop_resize(img, (0.0, 0.0, 4.0, 4.0), (4, 4))
    with pytest.raises(ValueError):
        I2G.crop_resize(img, (0, 0, 4, 4), (0, 4))
    with pytest.raises(ValueError):  # the second image is smaller than its box
        I2G.crop_resize([img, R.rand_img(4, 4)], [(0, 0, 10, 8), (0, 0, 5, 4)], (4, 4))
    with pytest.raises(TypeError):
        I2G.crop_resize(img.astype(np.float32), (0, 0, 4, 4), (4, 4))
    with pytest.raises(NotImplementedError):
        I2G.crop_resize(img, (0, 0, 4, 4), (4, 4), "lanczos")
    with pytest.raises(NotImplementedError):  # resize keeps refusing Image.resize's own box argument
        I2G.resize(img, (4, 4), box=(0, 0, 4, 4))


# ---- colour jitter -------------------------------------------------------------------------------------------------------------

RESIDENT = 128 * 128
JITTER_SIZES = [(1, 1), (1, 85), (85, 1), (16, 16), (37, 53), (128, 128), (129, 128), (131, 257)]


def _chains(B, seed):
    """B chains that walk through every order and the listed factors, some operations left to a factor of 1"""
    rng = np.random.default_rng(seed)
    order = np.array([R.ORDERS[(k + seed) % 6] for k in range(B)], np.int32)
    factors = np.array([[R.FACTORS[int(rng.integers(6))] for _ in range(3)] for _ in range(B)], np.float32)
    return order, factors


def _jitter_matches(imgs, factors, order, given=(True, True, True)):
    got = I2G.color_jitter(imgs, *[factors[:, op] if given[op] else None for op in range(3)], order=order)
    imgs = imgs.cpu().numpy() if isinstance(imgs, torch.Tensor) else imgs
    bad = []
    for b in range(len(imgs)):
        f = [float(factors[b, op]) if given[op] else None for op in range(3)]
        mism = _mismatch(got[b], R.pil_jitter(imgs[b], f, tuple(order[b])))
        if mism:
            bad.append((b, f, tuple(order[b]), mism))
    assert not bad, bad
    return got


def test_the_resident_limit_is_the_training_size():
    assert native.load_library().gnc_color_jitter_resident_pixels() == RESIDENT
    assert sum(h * w > RESIDENT for h, w in JITTER_SIZES) >= 2 and (128, 128) in JITTER_SIZES


@pytest.mark.parametrize("hw", JITTER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_color_jitter_equals_image_enhance(hw):
    B = 12
    imgs = np.stack([R.rand_img(*hw, seed=k) for k in range(B)])
    order, factors = _chains(B, seed=hw[0] + hw[1])
    src = torch.from_numpy(imgs).cuda()
    got = _jitter_matches(src, factors, order)
    assert got.data_ptr() != src.data_ptr() and np.array_equal(src.cpu().numpy(), imgs)  # a new tensor; the input is untouched


@pytest.mark.parametrize("order", R.ORDERS, ids=lambda o: "".join(map(str, o)))
def test_every_order_with_every_factor_pair(order):
    """all 36 (f_first, f_second) pairs of the listed factors on the first two operations of the order, the third drawn"""
    pairs = [(a, b) for a in R.FACTORS for b in R.FACTORS]
    rng = np.random.default_rng(5)
    factors = np.ones((len(pairs), 3), np.float32)
    for k, (a, b) in enumerate(pairs):
        factors[k, order[0]], factors[k, order[1]], factors[k, order[2]] = a, b, R.FACTORS[int(rng.integers(6))]
    imgs = np.stack([R.rand_img(16, 21, seed=k) for k in range(len(pairs))])
    _jitter_matches(imgs, factors, np.tile(np.array(order, np.int32), (len(pairs), 1)))


@pytest.mark.parametrize("given", [(True, False, False), (False, True, False), (False, False, True), (True, True, False),
                                   (False, True, True), (True, False, True)], ids=lambda g: "".join("bcs"[i] for i in range(3) if g[i]))
def test_operations_left_out(given):
    for hw in ((37, 53), (129, 128)):
        imgs = np.stack([R.rand_img(*hw, seed=k) for k in range(6)])
        order, factors = _chains(6, seed=sum(given))
        _jitter_matches(imgs, factors, order, given)


def test_special_images_and_scalar_factors():
    for hw in ((16, 16), (130, 128)):
        h, w = hw
        special = np.stack([np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), np.full((h, w, 3), 77, np.uint8),
                            R.half_mean_img(h, w, 100), R.half_mean_img(h, w, 254), R.half_mean_img(h, w, 0)])
        for f in R.FACTORS:
            got = I2G.color_jitter(special, contrast=f)
            for b in range(len(special)):
                assert _mismatch(got[b], R.pil_jitter(special[b], [None, f, None])) == 0, (hw, f, b)
        order, factors = _chains(len(special), seed=1)
        _jitter_matches(special, factors, order)
    # the k + 0.5 mean rounds up: contrast 0 paints the image k + 1
    assert (I2G.color_jitter(R.half_mean_img(16, 16, 100), contrast=0.0) == 101).all()
    assert (I2G.color_jitter(R.half_mean_img(130, 128, 100), contrast=0.0) == 101).all()


def test_factor_one_and_no_operation_return_the_input():
    for hw in ((37, 53), (129, 128)):
        imgs = np.stack([R.rand_img(*hw, seed=k) for k in range(3)])
        for order in R.ORDERS:
            assert _mismatch(I2G.color_jitter(imgs, 1.0, 1.0, 1.0, order=order), imgs) == 0
        assert _mismatch(I2G.color_jitter(imgs), imgs) == 0
        assert _mismatch(I2G.color_jitter(imgs[0], saturation=1.0), imgs[0]) == 0
        # a single image, and one operation beside two identities
        assert _mismatch(I2G.color_jitter(imgs[0], 1.0, 0.5, 1.0), R.pil_jitter(imgs[0], [1.0, 0.5, 1.0])) == 0


def test_color_jitter_rejects_bad_input():
    imgs = np.stack([R.rand_img(8, 8, seed=k) for k in range(2)])
    with pytest.raises(ValueError):
        I2G.color_jitter(imgs, brightness=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        I2G.color_jitter(imgs, brightness=-0.5)
    with pytest.raises(ValueError):
        I2G.color_jitter(imgs, brightness=0.5, order=[[0, 1, 1], [0, 1, 2]])
    with pytest.raises(ValueError):
        I2G.color_jitter(imgs, brightness=0.5, order=[[0, 1, 2]] * 3)
    with pytest.raises(ValueError):
        I2G.color_jitter(imgs[..., :2], brightness=0.5)
    with pytest.raises(TypeError):
        I2G.color_jitter(imgs.astype(np.float32), brightness=0.5)


# ---- the loaders ---------------------------------------------------------------------------------------------------------------

RES = 32


def _photo(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [127 + 120 * np.sin(xx / rng.uniform(5, 40) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(5, 40)) for _ in range(3)]
    return np.clip(np.stack(chans, -1) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("augment_images")
    shapes = [(60, 80), (75, 50), (64, 64), (40, 97), (33, 45), (90, 31)]
    for c, cls in enumerate(("ants", "bees")):
        os.makedirs(root / cls)
        for k, (h, w) in enumerate(shapes):
            Image.fromarray(_photo(h, w, 10 * c + k)).save(root / cls / f"{k}.jpg", quality=90)
    return str(root)


def _augmentation():
    return Augmentation(scale=(0.3, 1.0), brightness=0.4, contrast=0.4, saturation=0.4, seed=5)


def _pillow_images(ds, epoch, resample):
    decoded = [D.load_rgb(p) for p, _ in ds.samples]
    params = ds.augment.sample([im.shape[:2] for im in decoded], epoch, range(len(decoded)))
    return [R.pil_augment(im, params, b, ds.resize_value, resample) for b, im in enumerate(decoded)]


def _same_graphs(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u, v)


@pytest.mark.parametrize("method", ["pixel", "patch", "superpixel"])
def test_loader_graphs_equal_the_graphs_of_pillows_images(folder, method):
    kw = dict(resize_value=RES, method=method, n_segments=20, patch_size=4)
    ds = D.GraphImageFolder(folder, augment=_augmentation(), **kw)
    loader = ds.loader(shuffle=False, chunk=5)
    epochs = [[g for g, _ in loader] for _ in range(2)]
    for epoch, got in enumerate(epochs):
        want = I2G.graphs_from_images(_pillow_images(ds, epoch, "bicubic"), method, resize_value=RES, n_segments=20, patch_size=4)
        _same_graphs(got, want)
    assert any(a[0].shape != b[0].shape or not torch.equal(a[0], b[0]) for a, b in zip(*epochs))  # two epochs differ
    loader.set_epoch(0)
    _same_graphs([g for g, _ in loader], epochs[0])
    assert loader.epoch == 1
    # another chunk, a mini-batch size and a shuffle do not change a sample's augmentation
    torch.manual_seed(3)
    order = ds.loader(shuffle=True, batch_size=2).index_batches()
    assert order != [[i, i + 1] for i in range(0, len(ds), 2)]
    torch.manual_seed(3)  # the epoch below draws the same order
    for (batch, labels), idx in zip(ds.loader(shuffle=True, chunk=4, batch_size=2), order):
        for k, i in enumerate(idx):
            sub = batch.slice_graphs(k, k + 1)
            assert torch.equal(sub.x, epochs[0][i][0]) and torch.equal(sub.pos, epochs[0][i][1])
    # augment=False: the plain images, as a dataset without augment gives them; so does __getitem__
    plain = D.GraphImageFolder(folder, **kw)
    want = [g for g, _ in plain.loader(shuffle=False)]
    _same_graphs([g for g, _ in ds.loader(shuffle=False, augment=False)], want)
    _same_graphs([ds[i][0] for i in (0, 7)], [want[0], want[7]])


def test_tensor_folder_equals_pillows_images(folder):
    ds = D.ImageTensorFolder(folder, RES, augment=_augmentation())
    loader = ds.loader(batch_size=4, shuffle=False, chunk=8)
    epochs = [torch.cat([t for t, _ in loader]) for _ in range(2)]
    for epoch, got in enumerate(epochs):
        want = np.stack(_pillow_images(ds, epoch, "bilinear"))
        assert torch.equal(got.cpu(), torch.from_numpy(want).permute(0, 3, 1, 2).float().div(255))  # ToTensor, on the host
    assert not torch.equal(epochs[0], epochs[1])
    loader.set_epoch(1)
    assert torch.equal(torch.cat([t for t, _ in loader]), epochs[1])
    plain = torch.cat([t for t, _ in D.ImageTensorFolder(folder, RES).loader(batch_size=4, shuffle=False)])
    assert torch.equal(torch.cat([t for t, _ in ds.loader(batch_size=4, shuffle=False, augment=False)]), plain)
    assert torch.equal(ds[3][0], plain[3])


def test_training_on_an_augmented_pixel_folder_replays_the_captured_step(folder, tmp_path):
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    from graphnet_classifier_amd.train import train

    def run(augment, out):
        ds = D.GraphImageFolder(folder, resize_value=16, method="pixel", augment=augment)
        torch.manual_seed(0)
        model = CombinedModel(graph_net=GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3), num_nodes=256,
                              classes=2).cuda()
        torch.manual_seed(3)
        return train(model, ds.loader(chunk=6), 2, patience=5, output_path=str(tmp_path / out))

    plain, augmented = run(None, "plain"), run(_augmentation(), "augmented")
    assert plain["captured"] and augmented["captured"]
    assert len(augmented["avg_loss"]) == 2 and all(np.isfinite(v) for v in augmented["avg_loss"])
    assert augmented["avg_loss"] != plain["avg_loss"]  # the same order of samples, other pixels
