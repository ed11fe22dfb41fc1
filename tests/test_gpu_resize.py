"""GPU: the batched device resize (csrc/resize.hip) against live Pillow, byte for byte: degenerate and long-window
shapes, mixed-size batches, stream capture, and the argument checks."""
import numpy as np
import pytest
import torch
from PIL import Image

from graphnet_classifier_amd import image_to_graph as I2G

pytestmark = pytest.mark.gpu

PIL_FILTER = {"bicubic": Image.Resampling.BICUBIC, "bilinear": Image.Resampling.BILINEAR, "box": Image.Resampling.BOX}
# input (H, W) -> output (W, H)
CASES = [((1, 1), (1, 1)), ((1, 1), (7, 5)), ((1, 33), (8, 1)), ((1, 33), (40, 3)), ((29, 1), (1, 7)),
         ((29, 1), (4, 64)), ((24, 40), (40, 24)), ((16, 16), (32, 32)), ((64, 64), (32, 32)), ((37, 53), (101, 77)),
         ((97, 61), (23, 19)), ((50, 70), (70, 31)), ((50, 70), (13, 50)), ((375, 500), (128, 128)),
         ((1500, 2000), (128, 128)), ((3000, 4000), (64, 64))]


def _img(h, w, seed=0):
    return np.random.default_rng(seed * 100003 + h * 1009 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _pil(img, size, name="bicubic"):
    return np.array(Image.fromarray(img).resize(size, PIL_FILTER[name]))


@pytest.mark.parametrize("name", ["bicubic", "bilinear", "box"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-to-{c[1][1]}x{c[1][0]}")
def test_resize_equals_pillow(case, name):
    (h, w), size = case
    img = _img(h, w)
    got = I2G.resize(img, size, name)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (size[1], size[0], 3)
    want = _pil(img, size, name)
    mism = int((got.cpu().numpy() != want).sum())
    assert mism == 0, f"{mism} of {want.size} bytes differ"


def test_pil_resampling_values_are_accepted():
    img = _img(21, 34)
    for name, code in PIL_FILTER.items():
        assert np.array_equal(I2G.resize(img, (13, 8), code).cpu().numpy(), _pil(img, (13, 8), name))


@pytest.mark.parametrize("name", ["bicubic", "box"])
def test_mixed_size_batch_equals_per_image(name):
    shapes = [(375, 500), (1, 1), (128, 128), (129, 300), (77, 13), (64, 200), (500, 375), (128, 57)]
    imgs = [_img(h, w, seed=k) for k, (h, w) in enumerate(shapes)]
    batch = I2G.resize(imgs, (128, 96), name)
    assert tuple(batch.shape) == (len(imgs), 96, 128, 3)
    for k, img in enumerate(imgs):
        single = I2G.resize(img, (128, 96), name)
        assert torch.equal(batch[k], single), k
        assert np.array_equal(single.cpu().numpy(), _pil(img, (128, 96), name)), k
    # the same list with the images already on the device
    dev = I2G.resize([torch.from_numpy(im).cuda() for im in imgs], (128, 96), name)
    assert torch.equal(dev, batch)


def test_dense_batch_equals_per_image():
    imgs = np.stack([_img(90, 120, seed=k) for k in range(5)])
    for src in (imgs, torch.from_numpy(imgs), torch.from_numpy(imgs).cuda(), list(imgs)):
        out = I2G.resize(src, (64, 48))
        assert tuple(out.shape) == (5, 48, 64, 3)
        for k in range(5):
            assert np.array_equal(out[k].cpu().numpy(), _pil(imgs[k], (64, 48)))


def test_resize_replays_under_graph_capture():
    src = torch.from_numpy(np.stack([_img(200, 150, seed=k) for k in range(4)])).cuda()
    eager = I2G.resize(src, (128, 128))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        I2G.resize(src, (128, 128))  # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = I2G.resize(src, (128, 128))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    src.copy_(torch.from_numpy(np.stack([_img(200, 150, seed=10 + k) for k in range(4)])).cuda())
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, I2G.resize(src, (128, 128)))


def test_resize_rejects_bad_input():
    img = _img(8, 8)
    with pytest.raises(TypeError):
        I2G.resize(img.astype(np.float32), (4, 4))
    with pytest.raises(TypeError):
        I2G.resize(torch.zeros(8, 8, 3, dtype=torch.int32, device="cuda"), (4, 4))
    with pytest.raises(ValueError):
        I2G.resize(img[:, :, :2], (4, 4))
    with pytest.raises(ValueError):
        I2G.resize(np.zeros((2, 3, 8, 8, 3), np.uint8), (4, 4))
    with pytest.raises(ValueError):
        I2G.resize(np.zeros((0, 8, 3), np.uint8), (4, 4))
    with pytest.raises(ValueError):
        I2G.resize(np.zeros((0, 8, 8, 3), np.uint8), (4, 4))
    with pytest.raises(ValueError):
        I2G.resize([], (4, 4))
    with pytest.raises(ValueError):
        I2G.resize([img, np.zeros((4, 0, 3), np.uint8)], (4, 4))
    with pytest.raises(ValueError):
        I2G.resize(img, (0, 4))
    with pytest.raises(NotImplementedError):
        I2G.resize(img, (4, 4), "lanczos")
    with pytest.raises(NotImplementedError):
        I2G.resize(img, (4, 4), Image.Resampling.HAMMING)
