"""NumPy restatements of what csrc/augment.hip computes, and the Pillow calls they are pinned to.  Shared by the host and the GPU
tests of the augmentation (K25); nothing here needs a GPU."""
import itertools

import numpy as np
from PIL import Image, ImageEnhance

from tests.test_image_folder import PIL_FILTER, numpy_resize

ORDERS = list(itertools.permutations(range(3)))  # 0 brightness, 1 contrast, 2 saturation
ENHANCERS = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
# the issue's factors, rounded to float32 before they reach either side
FACTORS = [float(np.float32(f)) for f in (0.0, 0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, 2.0)]


def rand_img(h, w, seed=0):
    return np.random.default_rng(seed * 100003 + h * 1009 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def half_mean_img(h, w, k=100):
    """A two-tone grey image whose L mean is exactly k + 0.5: half the pixels k, half k + 1 (h * w must be even)."""
    assert (h * w) % 2 == 0
    flat = np.full(h * w, k, np.uint8)
    flat[1::2] = k + 1
    return np.repeat(flat.reshape(h, w, 1), 3, axis=2)


# ---- crop, resize, flip ------------------------------------------------------------------------------------------------------

def pil_crop_resize(img, box, size, name="bicubic", flip=False):
    out = Image.fromarray(img).crop(tuple(int(v) for v in box)).resize(size, PIL_FILTER[name])
    if flip:
        out = out.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    return np.array(out)


def numpy_crop_resize(img, box, size, name="bicubic", flip=False):
    """crop, THEN resize: the filter windows see nothing outside the box"""
    left, top, right, bottom = (int(v) for v in box)
    out = numpy_resize(img[top:bottom, left:right], size, name)
    return out[:, ::-1] if flip else out


# ---- colour jitter -----------------------------------------------------------------------------------------------------------

def luma(img):
    v = img.astype(np.int64)
    return (19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16


def blend(d, p, f):
    """Image.blend(degenerate, image, f) per byte: float32 with the multiply and the add rounded separately"""
    f = np.float32(f)
    v = d.astype(np.float32) + f * (p.astype(np.int64) - d.astype(np.int64)).astype(np.float32)
    assert v.dtype == np.float32
    return np.where(v <= 0, 0, np.where(v >= 255, 255, np.clip(v, 0, 255).astype(np.uint8))).astype(np.uint8)


def numpy_enhance(img, op, f):
    if op == 0:
        d = np.zeros(img.shape, np.int64)
    elif op == 1:
        lum = luma(img)
        mean = (2 * int(lum.sum()) + lum.size) // (2 * lum.size)
        d = np.full(img.shape, mean, np.int64)
    else:
        d = np.repeat(luma(img)[..., None], 3, axis=2)
    return blend(d, img, f)


def numpy_jitter(img, factors, order=(0, 1, 2)):
    """factors: (brightness, contrast, saturation), None = left out; order: the operations first to last"""
    out = img
    for op in order:
        if factors[op] is not None:
            out = numpy_enhance(out, op, factors[op])
    return out


def pil_jitter(img, factors, order=(0, 1, 2)):
    out = Image.fromarray(img)
    for op in order:
        if factors[op] is not None:
            out = ENHANCERS[op](out).enhance(float(np.float32(factors[op])))
    return np.array(out)


def pil_augment(img, params, b, size, name="bicubic"):
    """The image Pillow produces from sampled parameters (``augment.AugmentParams``) of sample b"""
    out = pil_crop_resize(img, params.boxes[b], (size, size), name, bool(params.flips[b]))
    factors = [None if f is None else float(f[b]) for f in (params.brightness, params.contrast, params.saturation)]
    return pil_jitter(out, factors, tuple(int(v) for v in params.order[b]))
