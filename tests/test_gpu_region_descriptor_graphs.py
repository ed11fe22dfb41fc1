"""GPU: ``node_features="descriptor"`` (DESIGN K26) through the layers above the kernel - the superpixel builders, the batched
build, ``graphs_from_images``, ``GraphImageFolder`` and its loaders, and a 16-column model forward, captured steps and ``train()``
on such graphs."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import graphnet_oracle as O
from tests._util import max_abs
from tests.test_superpixel_golden import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTH = {k: 32 for k in ("out_dim_node", "out_dim_edge", "hidden_dim_node", "hidden_dim_edge", "hidden_dim_decoder",
                         "hidden_dim_processor_node", "hidden_dim_processor_edge")}


@pytest.fixture(scope="module")
def I2G():
    from graphnet_classifier_amd import image_to_graph
    return image_to_graph


def _cases(shape, count=None):
    return [c for c in CASES if c[1].shape[:2] == shape][:count]


def _same(a, b):
    return all(torch.equal(s, t) and s.dtype == t.dtype for s, t in zip(a, b))


# --------------------------------------------------------------------------- builders
def test_batched_build_with_descriptors(I2G):
    cases = _cases((64, 64), 6)
    imgs, labs = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    plain = I2G.superpixel_graphs_batched(imgs, labs, node_capacity=160, edge_capacity=1280)
    wide = I2G.superpixel_graphs_batched(imgs, labs, node_capacity=160, edge_capacity=1280, node_features="descriptor")
    assert tuple(wide.x.shape) == (6, 160, 16) and tuple(plain.x.shape) == (6, 160, 3)
    assert torch.equal(wide.x[..., :3], plain.x) and torch.equal(wide.pos, plain.pos)
    assert torch.equal(wide.edge_index, plain.edge_index) and torch.equal(wide.counts, plain.counts)
    desc, counts = I2G.region_descriptors(imgs, labs, node_capacity=160)
    assert torch.equal(wide.x, desc) and torch.equal(counts[:, 0], plain.counts[:, 0])
    with pytest.raises(ValueError, match="Unknown node_features"):
        I2G.superpixel_graphs_batched(imgs, labs, node_capacity=160, edge_capacity=1280, node_features="mean")


def test_per_image_builders_with_descriptors(I2G, tmp_path):
    _, img, labs, params, _ = _cases((64, 64), 1)[0]
    x, pos, ei = I2G.superpixel_graph_from_labels(img, labs)
    wx, wpos, wei = I2G.superpixel_graph_from_labels(img, labs, node_features="descriptor")
    assert tuple(wx.shape) == (x.size(0), 16) and torch.equal(wx[:, :3], x) and torch.equal(wpos, pos) and torch.equal(wei, ei)
    assert torch.equal(wx, I2G.region_descriptors(img, labs)[0])
    plain = I2G.superpixel_graph_from_array(img)
    wide = I2G.superpixel_graph_from_array(img, node_features="descriptor")
    assert wide[0].size(1) == 16 and _same((wide[0][:, :3], wide[1], wide[2]), plain)
    seg = I2G.slic(img, n_segments=100, compactness=10, start_label=0)
    assert torch.equal(wide[0], I2G.region_descriptors(img, seg)[0])
    path = str(tmp_path / "one.png")
    Image.fromarray(img).save(path)
    assert _same(I2G.image_to_graph_superpixel(path, resize_value=64, node_features="descriptor"), wide)
    assert _same(I2G.image_to_graph_superpixel(path, resize_value=64), plain)


def test_graphs_from_images_batched_and_per_image_paths_agree(I2G):
    imgs = [c[1] for c in _cases((64, 64), 5)]
    want = [I2G.superpixel_graph_from_array(im, node_features="descriptor") for im in imgs]
    plain = I2G.graphs_from_images(imgs, method="superpixel", resize_value=64)
    low = sorted(int(g[0].size(0)) for g in want)[2]  # some of the images do not fit and take the per-image path
    for kw in ({}, {"node_capacity": low}, {"node_capacity": 1}, {"edge_capacity": 450}):
        got = I2G.graphs_from_images(imgs, method="superpixel", resize_value=64, node_features="descriptor", **kw)
        assert len(got) == 5
        for g, w, p in zip(got, want, plain):
            assert _same(g, w) and g[0].size(1) == 16 and g[0].is_contiguous()
            assert _same((g[0][:, :3], g[1], g[2]), p)
    knn = I2G.graphs_from_images(imgs, method="superpixel", resize_value=64, edges="knn", knn_k=6)
    for kw in ({}, {"node_capacity": 1}):
        wide = I2G.graphs_from_images(imgs, method="superpixel", resize_value=64, edges="knn", knn_k=6, node_features="descriptor", **kw)
        for g, w, p in zip(wide, want, knn):
            assert torch.equal(g[0], w[0]) and torch.equal(g[1], p[1]) and torch.equal(g[2], p[2])


def test_images_beyond_the_kernel_raise(I2G):
    with pytest.raises(NotImplementedError, match="512.*65536"):
        I2G.superpixel_graph_from_labels(np.zeros((257, 256, 3), np.uint8), np.zeros((257, 256), np.int32), node_features="descriptor")
    lab = np.arange(256, dtype=np.int32).reshape(16, 16)
    big = np.kron(lab, np.ones((2, 2), np.int32))  # 32 x 32, 256 regions: fine
    assert I2G.superpixel_graph_from_labels(np.zeros((32, 32, 3), np.uint8), big, node_features="descriptor")[0].shape == (256, 16)
    many = np.arange(32 * 32, dtype=np.int32).reshape(32, 32)  # 1024 regions
    with pytest.raises(NotImplementedError, match="512.*65536"):
        I2G.superpixel_graph_from_labels(np.zeros((32, 32, 3), np.uint8), many, node_features="descriptor")
    assert I2G.superpixel_graph_from_labels(np.zeros((32, 32, 3), np.uint8), many)[0].shape == (1024, 3)


# --------------------------------------------------------------------------- the folder
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """The eight 64 x 64 fixture photos in two classes (87 to 119 segments at the default parameters)."""
    root = tmp_path_factory.mktemp("photos")
    for k, case_id in enumerate(range(8, 16)):
        cid, img, _, _, _ = CASES[case_id]
        assert cid == case_id and img.shape == (64, 64, 3)
        cls = root / ("even" if k % 2 == 0 else "odd")
        os.makedirs(cls, exist_ok=True)
        Image.fromarray(img).save(cls / f"photo{k}.png")
    return str(root)


def test_folder_dataset_and_loaders_agree(I2G, folder):
    from graphnet_classifier_amd.dataset import GraphImageFolder, load_rgb
    ds = GraphImageFolder(folder, resize_value=64, method="superpixel", node_features="descriptor")
    base = GraphImageFolder(folder, resize_value=64, method="superpixel")
    assert ds.num_node_features == 16 and base.num_node_features == 3 and len(ds) == 8
    want = I2G.graphs_from_images([load_rgb(p) for p, _ in ds.samples], method="superpixel", resize_value=64, node_features="descriptor")
    single = [ds[i] for i in range(8)]
    stream = list(ds.loader(shuffle=False))
    plain = list(base.loader(shuffle=False))
    assert len(stream) == 8 and len({int(g[0].size(0)) for g, _ in stream}) >= 3
    for i in range(8):
        assert _same(single[i][0], want[i]) and _same(stream[i][0], want[i]) and int(single[i][1]) == int(stream[i][1]) == ds.samples[i][1]
        assert want[i][0].size(1) == 16 and _same((want[i][0][:, :3], want[i][1], want[i][2]), plain[i][0])
    batches = list(ds.loader(shuffle=False, batch_size=4))
    assert len(batches) == 2
    for k, (batch, labels) in enumerate(batches):
        ref = I2G.collate_graphs(want[4 * k:4 * k + 4])
        assert tuple(batch.x.shape) == (int(batch.graph_ptr[-1]), 16) and labels.tolist() == [t for _, t in ds.samples[4 * k:4 * k + 4]]
        assert torch.equal(batch.x, ref.x) and torch.equal(batch.pos, ref.pos) and torch.equal(batch.edge_index, ref.edge_index)
        assert torch.equal(batch.graph_ptr, ref.graph_ptr)


def test_folder_knn_edges_do_not_depend_on_the_features(folder):
    from graphnet_classifier_amd.dataset import GraphImageFolder
    kw = dict(resize_value=64, method="superpixel", edges="knn", knn_k=6)
    wide = list(GraphImageFolder(folder, node_features="descriptor", **kw).loader(shuffle=False))
    plain = list(GraphImageFolder(folder, **kw).loader(shuffle=False))
    for (g, _), (p, _) in zip(wide, plain):
        assert g[0].size(1) == 16 and torch.equal(g[0][:, :3], p[0]) and torch.equal(g[1], p[1]) and torch.equal(g[2], p[2])
        assert g[2].size(1) == 6 * g[0].size(0)


def test_folder_augmentation_is_in_front_of_the_descriptor(folder):
    from graphnet_classifier_amd.augment import Augmentation
    from graphnet_classifier_amd.dataset import GraphImageFolder
    aug = Augmentation(seed=7)
    kw = dict(resize_value=64, method="superpixel", augment=aug)
    wide, plain = GraphImageFolder(folder, node_features="descriptor", **kw).loader(shuffle=False), GraphImageFolder(folder, **kw).loader(shuffle=False)
    wide.set_epoch(3)
    plain.set_epoch(3)
    still = list(GraphImageFolder(folder, resize_value=64, method="superpixel").loader(shuffle=False))
    moved = 0
    for (g, _), (p, _), (s, _) in zip(wide, plain, still):
        assert g[0].size(1) == 16 and torch.equal(g[0][:, :3], p[0]) and torch.equal(g[1], p[1]) and torch.equal(g[2], p[2])
        moved += int(p[0].shape != s[0].shape or not torch.equal(p[0], s[0]))
    assert moved >= 6  # the augmentation did change the images


# --------------------------------------------------------------------------- the model on 16 columns
def _descriptor_graph(I2G, case):
    return I2G.superpixel_graph_from_labels(case[1], case[2], node_features="descriptor")


def _model(num_nodes, readout=None, ragged=False, seed=31):
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    torch.manual_seed(seed)
    gnet = GraphNet(num_local_features=16, space_dim=2, out_channels=1, n_blocks=2, **WIDTH)
    m = CombinedModel(gnet, num_nodes=num_nodes, classes=2) if readout is None else CombinedModel(gnet, num_nodes=num_nodes, classes=2, readout=readout)
    m.ragged_readout = ragged
    return m


def test_combined_model_on_a_descriptor_graph_matches_the_oracle(I2G):
    x, pos, ei = _descriptor_graph(I2G, _cases((32, 32), 1)[0])
    m = _model(int(x.size(0))).eval()
    with torch.no_grad():
        logits = m((x, pos, ei))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = O.combined_forward(sd, x.cpu(), pos.cpu(), ei.cpu())
    print(f"{x.size(0)} nodes x 16 columns: |logits - oracle| = {max_abs(logits.cpu(), ref):.3e}")
    assert logits.shape == (2,) and max_abs(logits.cpu(), ref) <= 1e-5


def _assert_gradients(got, ref, what):
    for k, r in ref.items():
        tol = 2e-5 + 1e-4 * float(r.abs().max())
        err = max_abs(got[k], r)
        assert got[k].shape == r.shape and err <= tol, f"{what}: {k} err {err:.3e} > {tol:.3e}"


def _eager_step(model_of, forward, label):
    """(loss, gradients, weights after the Adam step) of one eager step on a freshly seeded model"""
    from graphnet_classifier_amd.train import FlatParameters, FusedAdam
    e = model_of()
    eopt = FusedAdam(FlatParameters(e))
    loss = torch.nn.CrossEntropyLoss()(forward(e), label.to(DEV))
    eopt.zero_grad()
    loss.backward()
    eopt.fp.reducer()
    grads = {n: v.clone() for n, v in zip(eopt.fp.names, eopt.fp.reducer.views)}
    eopt.step()
    torch.cuda.synchronize()
    return float(loss.item()), grads, {k: v.detach().clone() for k, v in e.state_dict().items()}


def _assert_step(m, opt, loss_sum, loss, grads, after, what):
    """the bars of tests/test_gpu_superpixel_training.py (loss 1e-5 relative, 97 % of the weights within 2e-5) and of the captured
    steps' own tests (gradients within 2e-5 + 1e-4 max|ref|)"""
    torch.cuda.synchronize()
    got = float(loss_sum.item())
    print(f"{what}: captured loss {got:.8f}, eager {loss:.8f}")
    assert abs(got - loss) <= 1e-5 * max(1.0, abs(loss))
    _assert_gradients(dict(zip(opt.fp.names, opt.fp.reducer.views)), grads, what)
    close = total = 0
    for k, v in m.state_dict().items():
        d = (v - after[k]).abs()
        close += int((d <= 2e-5).sum())
        total += d.numel()
    print(f"{what}: weights within 2e-5: {close} of {total}")
    assert close >= 0.97 * total and int(opt.step_count.item()) == 1


def test_captured_any_size_step_on_descriptor_graphs(I2G):
    from graphnet_classifier_amd.train import CapturedTrainStep, FlatParameters, FusedAdam
    cases = _cases((64, 64))
    graphs = sorted((_descriptor_graph(I2G, c) for c in cases[:6]), key=lambda g: -int(g[0].size(0)))
    first, second = graphs[0], graphs[-1]
    assert first[0].size(0) > second[0].size(0) and first[0].size(1) == 16
    label = torch.tensor(1)
    model_of = lambda: _model(100, ragged=True)  # noqa: E731
    loss, grads, after = _eager_step(model_of, lambda e: e(second), label)
    m = model_of()
    opt = FusedAdam(FlatParameters(m))
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    step = CapturedTrainStep(m, opt, torch.nn.CrossEntropyLoss(), first, label, loss_sum, edge_capacity=1024, node_capacity=128)
    assert step.matches(first) and step.matches(second)
    assert not step.matches((second[0][:, :3].contiguous(), second[1], second[2]))  # three columns do not fit a 16-column capture
    step(second, label)
    step.check()
    _assert_step(m, opt, loss_sum, loss, grads, after, f"captured step, {second[0].size(0)} nodes after {first[0].size(0)}")


def test_captured_ragged_batch_step_on_descriptor_graphs(I2G):
    from graphnet_classifier_amd.train import CapturedRaggedBatchStep, FlatParameters, FusedAdam, padded_capacity
    cases = _cases((32, 32))
    assert len(cases) >= 8
    graphs = [_descriptor_graph(I2G, c) for c in cases[:8]]
    batches = [I2G.collate_graphs(graphs[:4]), I2G.collate_graphs(graphs[4:8])]
    labels = [torch.tensor([0, 1, 1, 0]), torch.tensor([1, 0, 1, 1])]
    E = padded_capacity(max(b.num_edges for b in batches))
    M = padded_capacity(max(b.num_nodes for b in batches), 0, 32)
    model_of = lambda: _model(32, readout="mean")  # noqa: E731
    b = batches[1]
    loss, grads, after = _eager_step(model_of, lambda e: e.forward_batched(b.x, b.pos, b.edge_index, graph_ptr=b.graph_ptr), labels[1])
    m = model_of()
    opt = FusedAdam(FlatParameters(m))
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    step = CapturedRaggedBatchStep(m, opt, torch.nn.CrossEntropyLoss(), batches[0], labels[0], loss_sum, edge_capacity=E, node_capacity=M)
    assert step.matches(batches[1])
    step(batches[1], labels[1])
    step.check()
    _assert_step(m, opt, loss_sum, loss, grads, after, f"captured batch step, {b.num_nodes} nodes x 16 columns")


def test_train_on_a_descriptor_folder(folder, tmp_path):
    from graphnet_classifier_amd.dataset import GraphImageFolder
    from graphnet_classifier_amd.train import evaluate, train
    ds = GraphImageFolder(folder, resize_value=64, method="superpixel", node_features="descriptor")
    m = _model(100, ragged=True)
    r = train(m, ds.loader(shuffle=False), 2, patience=5, output_path=str(tmp_path / "w"))
    assert r["captured_ragged"] is True and len(r["avg_loss"]) == 2 and all(np.isfinite(v) for v in r["avg_loss"])
    ev = evaluate(m.eval(), ds.loader(shuffle=False, augment=False))
    assert ev["count"] == 8 and np.isfinite(ev["loss"])
