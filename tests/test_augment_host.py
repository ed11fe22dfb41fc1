"""CPU: the rules of the device augmentation (K25) pinned to live Pillow through their NumPy restatement, the sampling of
``augment.Augmentation``, and the C ABI of csrc/augment.hip.  No GPU is needed."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from graphnet_classifier_amd import dataset as D
from graphnet_classifier_amd import native
from graphnet_classifier_amd.augment import ORDERS, Augmentation, central_crop
from tests import augment_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images():
    return {"random": R.rand_img(23, 31), "constant": np.full((9, 14, 3), 77, np.uint8), "zeros": np.zeros((8, 8, 3), np.uint8),
            "ones": np.full((8, 8, 3), 255, np.uint8), "half": R.half_mean_img(6, 10, 100),
            "tinted": np.broadcast_to(np.array([200, 30, 90], np.uint8), (5, 7, 3)).copy()}


def test_half_mean_image_has_an_l_mean_of_exactly_k_plus_a_half():
    lum = R.luma(R.half_mean_img(6, 10, 100))
    assert lum.sum() * 2 == (2 * 100 + 1) * lum.size
    # ... which Contrast rounds up: int(mean + 0.5) = k + 1; with f = 0 every byte becomes that grey level
    assert (R.pil_jitter(R.half_mean_img(6, 10, 100), [None, 0.0, None]) == 101).all()


@pytest.mark.parametrize("order", R.ORDERS, ids=lambda o: "".join(map(str, o)))
def test_numpy_jitter_equals_pillow_for_every_order_and_factor(order):
    rng = np.random.default_rng(sum(order[i] * 3 ** i for i in range(3)))
    for name, img in _images().items():
        for f0 in R.FACTORS:
            for f1 in R.FACTORS:
                f2 = R.FACTORS[int(rng.integers(len(R.FACTORS)))]
                factors = [f0, f1, f2]
                assert np.array_equal(R.numpy_jitter(img, factors, order), R.pil_jitter(img, factors, order)), (name, factors)


def test_numpy_jitter_single_operations_and_identity():
    for name, img in _images().items():
        for op in range(3):
            for f in R.FACTORS + [float(np.float32(0.3)), float(np.float32(1.7))]:
                factors = [None] * 3
                factors[op] = f
                assert np.array_equal(R.numpy_jitter(img, factors), R.pil_jitter(img, factors)), (name, op, f)
        assert np.array_equal(R.numpy_jitter(img, [1.0, 1.0, 1.0]), img)
        assert np.array_equal(R.pil_jitter(img, [1.0, 1.0, 1.0]), img)


def test_numpy_jitter_equals_pillow_for_random_float32_factors():
    rng = np.random.default_rng(0)
    for t in range(120):
        img = R.rand_img(12 + t % 5, 17, seed=t)
        factors = [float(np.float32(rng.uniform(0, 2))) for _ in range(3)]
        assert np.array_equal(R.numpy_jitter(img, factors, R.ORDERS[t % 6]), R.pil_jitter(img, factors, R.ORDERS[t % 6])), factors


@pytest.mark.parametrize("name", ["bicubic", "bilinear", "box"])
def test_numpy_crop_resize_equals_pillow_and_is_not_resize_with_a_box(name):
    img = R.rand_img(37, 53)
    differs = 0
    for box, size in [((0, 0, 53, 37), (20, 20)), ((3, 5, 40, 30), (16, 24)), ((1, 0, 2, 37), (5, 9)), ((0, 7, 53, 8), (11, 3)),
                      ((10, 10, 11, 11), (4, 4)), ((2, 3, 18, 19), (16, 16)), ((5, 1, 53, 37), (64, 48))]:
        for flip in (False, True):
            assert np.array_equal(R.numpy_crop_resize(img, box, size, name, flip), R.pil_crop_resize(img, box, size, name, flip))
        inside = np.array(Image.fromarray(img).resize(size, R.PIL_FILTER[name], box=box))
        differs += int((inside != R.pil_crop_resize(img, box, size, name)).any())
    if name != "box":  # (a BOX window never leaves an integer box)
        assert differs > 0  # Image.resize(box=...) reads outside the box: another function


# ---- sampling ------------------------------------------------------------------------------------------------------------------

SIZES = [(375, 500), (500, 375), (128, 128), (1, 300), (300, 1), (64, 200), (33, 17), (1, 1), (240, 320), (90, 90)]


def _aug(**kw):
    return Augmentation(brightness=0.4, contrast=0.4, saturation=(0.5, 1.5), seed=7, **kw)


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def test_parameters_depend_on_seed_epoch_and_index_alone():
    aug, idx = _aug(), list(range(len(SIZES)))
    whole = aug.sample(SIZES, 3, idx)
    # chunked, and in another order of the request
    parts = [aug.sample(SIZES[i:i + 3], 3, idx[i:i + 3]) for i in range(0, len(idx), 3)]
    for field in range(6):
        assert np.array_equal(np.concatenate([p[field] for p in parts]), whole[field])
    perm = [7, 2, 9, 0, 4, 1, 8, 3, 6, 5]
    shuffled = aug.sample([SIZES[i] for i in perm], 3, perm)
    for field in range(6):
        assert np.array_equal(shuffled[field], whole[field][perm])
    assert _same(_aug().sample(SIZES, 3, idx), whole)
    other_epoch, other_seed = aug.sample(SIZES, 4, idx), Augmentation(brightness=0.4, contrast=0.4, saturation=(0.5, 1.5), seed=8)
    assert not np.array_equal(other_epoch.boxes, whole.boxes) and not np.array_equal(other_epoch.brightness, whole.brightness)
    assert not np.array_equal(other_seed.sample(SIZES, 3, idx).boxes, whole.boxes)
    # the sample index, not the position in the request, is the key
    assert not np.array_equal(aug.sample(SIZES, 3, [i + 100 for i in idx]).boxes, whole.boxes)


def test_boxes_lie_inside_their_images_and_factors_in_their_ranges():
    aug = _aug()
    for epoch in range(20):
        p = aug.sample(SIZES, epoch, range(len(SIZES)))
        for (h, w), (left, top, right, bottom) in zip(SIZES, p.boxes):
            assert 0 <= left < right <= w and 0 <= top < bottom <= h
        assert p.boxes.dtype == np.int64 and p.flips.dtype == bool and p.order.dtype == np.int32
        for f, (lo, hi) in ((p.brightness, (0.6, 1.4)), (p.contrast, (0.6, 1.4)), (p.saturation, (0.5, 1.5))):
            assert f.dtype == np.float32 and (f >= np.float32(lo)).all() and (f <= np.float32(hi)).all()
        assert all(tuple(o) in ORDERS for o in p.order)
    flips = np.concatenate([aug.sample(SIZES, e, range(len(SIZES))).flips for e in range(40)])
    assert 0.35 < flips.mean() < 0.65


def test_crop_follows_the_random_resized_crop_rule():
    """A try fits on a square image: the box then has an area within scale and a ratio within ratio (up to rounding)."""
    aug = Augmentation(scale=(0.25, 0.5), ratio=(0.5, 2.0), seed=1)
    p = aug.sample([(200, 200)] * 50, 0, range(50))
    w, h = p.boxes[:, 2] - p.boxes[:, 0], p.boxes[:, 3] - p.boxes[:, 1]
    assert ((w * h >= 0.25 * 40000 * 0.97) & (w * h <= 0.5 * 40000 * 1.03)).all()
    assert ((w / h > 0.5 * 0.97) & (w / h < 2.0 * 1.03)).all()
    assert len({tuple(b) for b in p.boxes}) > 40


def test_an_image_no_try_fits_takes_the_central_crop():
    aug = Augmentation(seed=3)
    for epoch in range(5):
        p = aug.sample([(1, 300), (300, 1)], epoch, [0, 1])
        assert tuple(p.boxes[0]) == (149, 0, 150, 1)  # ratio clamped to 4/3: w = round(1 * 4/3) = 1, centred
        assert tuple(p.boxes[1]) == (0, 149, 1, 150)  # ratio clamped to 3/4: h = round(1 / (3/4)) = 1, centred
    assert central_crop(100, 400, (0.75, 4 / 3)) == (133, 0, 266, 100)  # w = round(100 * 4/3) = 133
    assert central_crop(400, 100, (0.75, 4 / 3)) == (0, 133, 100, 266)
    assert central_crop(100, 120, (0.75, 4 / 3)) == (0, 0, 120, 100)


def test_switches():
    off = Augmentation(scale=None, hflip=0, seed=0).sample(SIZES, 0, range(len(SIZES)))
    assert all(tuple(b) == (0, 0, w, h) for b, (h, w) in zip(off.boxes, SIZES)) and not off.flips.any()
    assert off.brightness is None and off.contrast is None and off.saturation is None
    only = Augmentation(contrast=0.2).sample(SIZES, 0, range(len(SIZES)))
    assert only.brightness is None and only.saturation is None and only.contrast is not None
    assert Augmentation(hflip=1.0).sample(SIZES, 0, range(len(SIZES))).flips.all()
    for bad in (dict(scale=(0.0, 1.0)), dict(ratio=(2.0, 1.0)), dict(hflip=1.5), dict(brightness=-0.1), dict(contrast=(1.5, 0.5))):
        with pytest.raises(ValueError):
            Augmentation(**bad)
    with pytest.raises(ValueError):
        Augmentation().sample(SIZES, 0, [0])


def _folder(tmp_path, n=6):
    for cls in ("a", "b"):
        os.makedirs(tmp_path / cls)
        for k in range(n):
            Image.fromarray(R.rand_img(20 + k, 30 - k, seed=k)).save(tmp_path / cls / f"{k}.png")
    return str(tmp_path)


def test_sampling_leaves_the_global_rng_alone_and_the_order_is_unchanged(tmp_path):
    torch.manual_seed(11)
    before = torch.get_rng_state()
    _aug().sample(SIZES, 0, range(len(SIZES)))
    assert torch.equal(torch.get_rng_state(), before)
    root = _folder(tmp_path)
    plain, augmented = D.GraphImageFolder(root, 16), D.GraphImageFolder(root, 16, augment=_aug())
    orders = []
    for ds, kw in ((plain, {}), (augmented, {}), (augmented, {"augment": False})):
        torch.manual_seed(5)
        loader = ds.loader(**kw)
        orders.append((loader.order(), loader.order(), torch.get_rng_state()))
    for other in orders[1:]:
        assert other[0] == orders[0][0] and other[1] == orders[0][1] and torch.equal(other[2], orders[0][2])
    assert augmented.loader().augment is augmented.augment and augmented.loader(augment=False).augment is None
    assert plain.loader().augment is None
    loader = augmented.loader()
    assert loader.epoch == 0
    loader.set_epoch(5)
    assert loader._next_epoch() == 5 and loader.epoch == 6
    with pytest.raises(TypeError):
        D.GraphImageFolder(root, 16, augment="yes")
    with pytest.raises(TypeError):
        D.ImageTensorFolder(root, 16, augment=True)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------

def test_augment_symbols_are_declared_exported_and_bound():
    lib = native.load_library()
    header = open(os.path.join(ROOT, "include", "gnc_hip.h")).read()
    for name, ret in (("gnc_crop_resize_workspace_bytes", "size_t"), ("gnc_crop_resize_rgb_u8", "int"),
                      ("gnc_color_jitter_resident_pixels", "int64_t"), ("gnc_color_jitter_rgb_u8", "int")):
        assert name in native._SIGNATURES and name in native.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header), name
    # the crop's workspace is the resize's (a box lies in its image); 0 says "outside the supported set"
    for args in ((8, 375, 500, 128, 128, 3), (1, 1, 1, 1, 1, 4), (64, 3000, 4000, 64, 64, 2)):
        assert lib.gnc_crop_resize_workspace_bytes(*args) == lib.gnc_resize_workspace_bytes(*args) > 0
    assert lib.gnc_crop_resize_workspace_bytes(1, 70000, 8, 8, 8, 3) == 0
    assert lib.gnc_crop_resize_workspace_bytes(1, 8, 8, 8, 8, 1) == 0
    assert lib.gnc_color_jitter_resident_pixels() >= 128 * 128  # a 128 x 128 training image stays on chip


def test_bad_arguments_are_refused_before_any_hip_call():
    lib = native.load_library()
    assert lib.gnc_crop_resize_rgb_u8(None, None, None, 1, 8, 8, 4, 4, 3, None, None, 0, None) != 0
    assert b"null pointer" in lib.gnc_last_error_string()
    assert lib.gnc_color_jitter_rgb_u8(None, 1, 8, 8, None, None, None) != 0
    assert b"null pointer" in lib.gnc_last_error_string()
