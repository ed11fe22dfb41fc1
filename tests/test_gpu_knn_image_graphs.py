"""GPU: ``edges="knn"`` through ``graphs_from_images`` / ``GraphImageFolder`` and its loader (DESIGN K24) - the nodes stay the
method's own bit for bit, the edges equal the NumPy reference on the features read back from ``knn_features`` (so nothing here
depends on how ``torch`` rounds the scaling), the loader's graphs equal ``__getitem__``'s, and ``train()`` takes the graphs as
they are.  The existing batched-build test does not count host synchronisations, so the superpixel chunk is compared with the
per-image path instead."""
import copy
import os

import numpy as np
import pytest
import torch
from PIL import Image

from graphnet_classifier_amd import dataset as D
from graphnet_classifier_amd import image_to_graph as I2G
from tests import knn_reference as R

pytestmark = pytest.mark.gpu

CONFIGS = {
    "pixel": dict(resize_value=16, knn_k=8),
    "patch": dict(resize_value=32, patch_size=8, knn_k=4),  # 16 nodes
    "superpixel": dict(resize_value=64, n_segments=30, knn_k=8),
}


def _photo(h, w, seed):
    """smooth colour fields with some noise, as tests/test_gpu_image_folder.py draws them"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [127 + 120 * np.sin(xx / rng.uniform(5, 40) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(5, 40)) for _ in range(3)]
    return np.clip(np.stack(chans, -1) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("knn_images")
    shapes = [(150, 200), (128, 128), (90, 333), (64, 64), (97, 211), (257, 129)]
    for i, (h, w) in enumerate(shapes):
        cls = root / ("ants" if i % 2 == 0 else "bees")
        os.makedirs(cls, exist_ok=True)
        Image.fromarray(_photo(h, w, i + 1)).save(cls / f"im{i}.png")
    return str(root)


def _reference_edges(x, pos, method, cfg, pos_weight=1.0):
    feat = I2G.knn_features(x, pos, method, cfg["resize_value"], pos_weight)
    assert feat.dtype == torch.float32 and tuple(feat.shape) == (x.size(0), 5)
    return R.knn_graph(feat.cpu().numpy(), cfg["knn_k"])[0]


@pytest.mark.parametrize("method", ["pixel", "patch", "superpixel"])
def test_knn_edges_over_the_methods_own_nodes(folder, method):
    cfg = CONFIGS[method]
    plain = D.GraphImageFolder(folder, method=method, **{k: v for k, v in cfg.items() if k != "knn_k"})
    knn = D.GraphImageFolder(folder, method=method, edges="knn", **cfg)
    assert len(knn) == 6
    items = []
    for i in range(len(knn)):
        (x, pos, ei), label = knn[i]
        (px, ppos, pei), plabel = plain[i]
        assert torch.equal(x, px) and torch.equal(pos, ppos) and int(label) == int(plabel)  # the nodes are untouched
        n, k = x.size(0), cfg["knn_k"]
        assert ei.dtype == torch.int64 and ei.is_cuda and tuple(ei.shape) == (2, k * n) and ei.is_contiguous()
        assert np.array_equal(ei.cpu().numpy(), _reference_edges(x, pos, method, cfg))
        if method == "patch":
            assert n == 16
        items.append((x, pos, ei))
    seen = 0
    for chunk in (4, 64):  # several chunks, and the whole folder in one
        for i, ((x, pos, ei), label) in enumerate(knn.loader(shuffle=False, chunk=chunk)):
            wx, wpos, wei = items[i]
            assert torch.equal(x, wx) and torch.equal(pos, wpos) and torch.equal(ei, wei)
            seen += 1
    assert seen == 12


def test_superpixel_chunk_equals_the_per_image_path(folder):
    cfg = CONFIGS["superpixel"]
    ds = D.GraphImageFolder(folder, method="superpixel", edges="knn", **cfg)
    images = [D.load_rgb(p) for p, _ in ds.samples]
    kw = dict(method="superpixel", resize_value=64, n_segments=30, edges="knn", knn_k=8)
    batched = I2G.graphs_from_images(images, **kw)
    sizes = sorted(int(g[0].size(0)) for g in batched)
    assert sizes[0] > 8
    # a node capacity in the middle: some images overflow it and take the per-image path; 513 is outside the batched kernel's set
    for extra in ({"node_capacity": sizes[3]}, {"node_capacity": 513}):
        mixed = I2G.graphs_from_images(images, **kw, **extra)
        for a, b in zip(batched, mixed):
            assert all(torch.equal(u, v) for u, v in zip(a, b))
    x, pos, _ = batched[0]
    assert torch.equal(I2G.knn_edges(x, pos, 8, "superpixel", 64), batched[0][2])
    with pytest.raises(ValueError, match="knn_k"):
        I2G.graphs_from_images(images, **{**kw, "knn_k": 16, "n_segments": 8})


def test_pos_weight_moves_between_colour_and_space(folder):
    cfg = CONFIGS["patch"]
    images = [D.load_rgb(p) for p, _ in D.GraphImageFolder(folder, method="patch").samples]
    kw = dict(method="patch", resize_value=32, patch_size=8, edges="knn", knn_k=4)
    colour = I2G.graphs_from_images(images, **kw, knn_pos_weight=0.0)
    space = I2G.graphs_from_images(images, **kw, knn_pos_weight=1e6)
    assert any(not torch.equal(c[2], s[2]) for c, s in zip(colour, space))
    for (x, pos, ei), (cx, cpos, cei) in zip(space, colour):
        # positions are multiples of 1/64 of the image: pos / 32 * 1e6 is exact, and a squared step of it (>= 6e10, an ulp of
        # 4096 or more) swallows the colour terms (at most 3) whole - the distance IS the spatial one, ties and all
        assert np.array_equal(ei.cpu().numpy(), R.knn_graph(pos.cpu().numpy(), 4)[0])
        assert np.array_equal(cei.cpu().numpy(), R.knn_graph((cx / 255.0).cpu().numpy(), 4)[0])


def test_train_takes_knn_graphs_as_they_are(folder, tmp_path):
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    from graphnet_classifier_amd.train import train
    ds = D.GraphImageFolder(folder, method="superpixel", edges="knn", **CONFIGS["superpixel"])
    torch.manual_seed(0)
    model = CombinedModel(GraphNet(**synthetic.graphnet_kwargs(64, 2)), num_nodes=100, classes=2, readout="mean").cuda()
    twin = copy.deepcopy(model)
    sample, label = ds[0]
    with torch.no_grad():
        eager = float(torch.nn.CrossEntropyLoss()(model(sample).reshape(1, -1), label.reshape(1).cuda()))
    first = train(twin, [(sample, label)], 1, patience=5, output_path=str(tmp_path / "one"))
    print("first-step loss", first["avg_loss"][0], "eager forward", eager)
    assert abs(first["avg_loss"][0] - eager) <= 1e-5 * max(1.0, abs(eager))
    torch.manual_seed(1)
    r = train(model, ds.loader(), 2, patience=5, output_path=str(tmp_path / "run"))
    print({k: v for k, v in r.items() if k.startswith("captured")}, r["avg_loss"])
    assert r["captured_any_topology"], "the padded capture did not take the kNN graphs"
    assert len(r["avg_loss"]) == 2 and all(np.isfinite(v) for v in r["avg_loss"])
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
