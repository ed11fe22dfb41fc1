"""GPU: mini-batch training and evaluation from an image folder - ``GraphImageFolder.loader(batch_size=B)`` ->
``train()`` -> ``evaluate()`` / ``predict()`` - against a CPU loop over the float64 oracle (``oracle.combined_forward`` per graph,
mean cross-entropy over the batch, ``torch.optim.Adam(lr=1e-3)``), captured against eager, and the unchanged ``batch_size=1``
loader.  The folder: 10 generated PNGs in 2 classes."""
import numpy as np
import pytest
import torch
from PIL import Image

from oracle import graphnet_oracle as O
from tests import readout_batched_cases as R
from tests._util import max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _folder(root, side=16, count=10, smooth=False):
    """``smooth``: low-frequency colour fields instead of per-pixel noise (SLIC's connectivity pass merges the fragments of a
    noise image into a handful of segments; smooth images keep about ``n_segments`` of them, a few more or less per image)."""
    rng = np.random.default_rng(2024)
    for k in range(count):
        yy, xx = np.mgrid[0:side, 0:side]
        if smooth:
            f = rng.uniform(0.5, 2.5, size=(3, 2)) * (2 * np.pi / side)
            ph = rng.uniform(0, 2 * np.pi, size=(3, 2))
            img = np.stack([127 + 60 * np.sin(f[c, 0] * yy + ph[c, 0]) + 60 * np.sin(f[c, 1] * xx + ph[c, 1]) for c in range(3)],
                           axis=-1).astype(np.uint8)
        else:
            img = rng.integers(0, 256, size=(side, side, 3), dtype=np.uint8)
        c = k % 2
        # class 0: a bright disc whose place and size change per image, class 1: stripes of a changing period
        mask = ((yy - side * (0.3 + 0.04 * k)) ** 2 + (xx - side * 0.5) ** 2 < (side * (0.2 + 0.02 * k)) ** 2) if c == 0 \
            else ((xx // (2 + k // 2)) % 2 == 0)
        img[mask] = (img[mask] // 4 + np.array([190, 40 + 15 * k, 60], dtype=np.uint8)).astype(np.uint8)
        d = root / f"class{c}"
        d.mkdir(parents=True, exist_ok=True)
        Image.fromarray(img).save(d / f"img{k:02d}.png")
    return str(root)


def _model(num_nodes, ragged=False):
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    torch.manual_seed(99)
    m = CombinedModel(GraphNet(**synthetic.graphnet_kwargs(32, 1)), num_nodes=num_nodes, classes=2)
    m.ragged_readout = ragged
    return m


def _cpu_graphs(ds):
    """Every image's graph and label in dataset order, as CPU tensors."""
    return [(tuple(t.cpu() for t in g), int(lab)) for g, lab in ds.loader(shuffle=False)]


def _oracle_training(sd0, graphs, epochs_batches, num_nodes):
    """The reference loop in float64 on the CPU: per batch the oracle's logits per graph (zero-padding rule for a graph whose
    node count is not ``num_nodes``), mean CE, Adam(lr=1e-3); the epoch average over steps (utils/train_model.py:47).
    ``epochs_batches``: the index batches of every epoch."""
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-3)
    O.set_scatter_impl("index_add")  # the differentiable form of the oracle's scatter
    history = []
    try:
        for batches in epochs_batches:
            total = 0.0
            for idx in batches:
                logits = []
                for i in idx:
                    (x, pos, ei), _ = graphs[i]
                    y = O.graphnet_forward(params, x, pos, ei, prefix="graph_net.")
                    logits.append(O.classifier_forward(params, R.gather_features(y, torch.tensor([0, y.size(0)]), num_nodes)[0]))
                loss = torch.nn.functional.cross_entropy(torch.stack(logits), torch.tensor([graphs[i][1] for i in idx]))
                opt.zero_grad()
                loss.backward()
                opt.step()
                total += float(loss.detach())
            history.append(total / len(batches))
    finally:
        O.set_scatter_impl("sorted_loop")
    return history, {k: v.detach() for k, v in params.items()}


def test_pixel_minibatches_match_the_oracle_loop(tmp_path):
    """Shuffled mini-batches of 4, as main.py feeds its loaders (``shuffle=True``): 2 full batches replay the captured step, the
    short third one runs eagerly; the oracle loop walks the same index batches (``index_batches`` under the same seed).
    Measured: losses within 6.1e-8 of the oracle's, final parameters within 6.2e-6.

    Not ``shuffle=False``: the folder order is class by class, and on THESE images a step on the one-class first batch leaves a
    few parameters with gradients at rounding level, which Adam turns into moves of 3e-6 in a direction fp32 noise decides; one
    ReLU of the node decoder then comes out on the other side in the second step (loss still equal to 1.7e-8, that layer's
    gradient off by 4e-4) and the run leaves the float64 one (4e-5 in the second epoch's loss) - with ``torch.optim.Adam``
    and the torch read-out just the same.  A property of fp32 against float64 on that batch order, not of the batched path."""
    from graphnet_classifier_amd.dataset import GraphImageFolder
    from graphnet_classifier_amd.train import train
    ds = GraphImageFolder(_folder(tmp_path / "data"), resize_value=16, method="pixel")
    graphs = _cpu_graphs(ds)
    assert len(graphs) == 10 and all(g[0][0].size(0) == 256 for g in graphs)
    m = _model(256)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    loader = ds.loader(shuffle=True, batch_size=4)
    assert len(loader) == 3
    torch.manual_seed(0)
    epochs_batches = [loader.index_batches() for _ in range(2)]
    assert [len(b) for b in epochs_batches[0]] == [4, 4, 2] and epochs_batches[0] != epochs_batches[1]
    torch.manual_seed(0)
    r = train(m, loader, 2, patience=5, output_path=str(tmp_path / "run"))
    ref_loss, ref_sd = _oracle_training(sd0, graphs, epochs_batches, 256)
    print("avg_loss", r["avg_loss"], "oracle", ref_loss)
    assert r["batched"] is True and r["captured"] is True
    assert len(r["avg_loss"]) == 2 and max(abs(a - b) for a, b in zip(r["avg_loss"], ref_loss)) <= 1e-5
    # 6 Adam steps: an entry whose gradient is at rounding level moves by ~lr per step in a direction fp32 noise decides (the
    # bound of test_train_reproduces_the_reference_run, per step); everything else agrees to rounding
    final = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    worst = max(max_abs(final[k], ref_sd[k]) for k in final)
    close = np.mean([float(((final[k].double() - ref_sd[k]).abs() < 2e-5).float().mean()) for k in final])
    print(f"final parameters: worst {worst:.3e}, fraction within 2e-5: {close:.4f}")
    assert worst < 6 * 2.1e-3 and close > 0.97
    lines = open(r["log_path"]).read().splitlines()
    assert [l for l in lines if "avg_loss=" in l] == [f"Epoch {k + 1}/2, avg_loss={v:.4f}" for k, v in enumerate(r["avg_loss"])]


def test_captured_minibatch_training_equals_eager(tmp_path):
    from graphnet_classifier_amd.dataset import GraphImageFolder
    from graphnet_classifier_amd.train import train
    ds = GraphImageFolder(_folder(tmp_path / "data"), resize_value=16, method="pixel")
    out = {}
    for capture in (False, True):
        m = _model(256)
        torch.manual_seed(3)  # the same shuffled batches in both runs
        r = train(m, ds.loader(shuffle=True, batch_size=4), 2, patience=5, output_path=str(tmp_path / str(capture)), capture=capture)
        assert r["batched"] and r["captured"] == capture
        out[capture] = ({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, r["avg_loss"])
    assert out[True][1] == out[False][1]
    for k in out[True][0]:
        assert torch.equal(out[True][0][k], out[False][0][k]), k


def test_captured_minibatch_training_through_graph_ptr_equals_eager(tmp_path):
    """The twin of the test above on a model with ``ragged_readout``: its mini-batch step takes the ``graph_ptr`` form of
    ``forward_batched``, whose device offsets only the ``forward=`` closure of the captured step holds.  Batches of 4, 4, 2 over two
    epochs: the short batch runs eagerly - and allocates - between the first epoch's replay and the second epoch's two, so
    offsets that the capture did not keep alive would be somebody else's bytes by then."""
    from graphnet_classifier_amd.dataset import GraphImageFolder
    from graphnet_classifier_amd.train import train
    ds = GraphImageFolder(_folder(tmp_path / "data"), resize_value=8, method="pixel")
    out = {}
    for capture in (False, True):
        m = _model(64, ragged=True)
        torch.manual_seed(3)  # the same shuffled batches in both runs
        loader = ds.loader(shuffle=True, batch_size=4)
        assert len(loader) == 3
        r = train(m, loader, 2, patience=5, output_path=str(tmp_path / str(capture)), capture=capture)
        assert r["batched"] and r["captured"] == capture
        out[capture] = ({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, r["avg_loss"])
    print("avg_loss captured", out[True][1], "eager", out[False][1])
    print("final parameters: worst |captured - eager| =", max(max_abs(out[True][0][k], out[False][0][k]) for k in out[True][0]))
    assert out[True][1] == out[False][1]
    for k in out[True][0]:
        assert torch.equal(out[True][0][k], out[False][0][k]), k


def test_batch_size_one_is_the_loader_it_was(tmp_path):
    from graphnet_classifier_amd.dataset import GraphImageFolder
    ds = GraphImageFolder(_folder(tmp_path / "data"), resize_value=16, method="pixel")
    torch.manual_seed(8)
    old = list(ds.loader(shuffle=True))
    state = torch.get_rng_state()
    torch.manual_seed(8)
    new = list(ds.loader(shuffle=True, batch_size=1, drop_last=False))
    assert torch.equal(torch.get_rng_state(), state) and len(old) == len(new) == 10
    for (g0, l0), (g1, l1) in zip(old, new):
        assert isinstance(g1, tuple) and len(g1) == 3 and l1.dim() == 0 and torch.equal(l0, l1)
        assert all(torch.equal(a, b) for a, b in zip(g0, g1))


def test_collated_batches_are_the_loaders_graphs(tmp_path):
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.dataset import GraphImageFolder
    ds = GraphImageFolder(_folder(tmp_path / "data"), resize_value=16, method="pixel")
    graphs = _cpu_graphs(ds)
    seen = 0
    for batch, labels in ds.loader(shuffle=False, batch_size=4, drop_last=True):
        assert isinstance(batch, synthetic.GraphBatch) and batch.x.is_cuda and labels.shape == (4,)
        for g in range(batch.num_graphs):
            b = batch.slice_graphs(g, g + 1)
            (x, pos, ei), lab = graphs[seen]
            assert torch.equal(b.x.cpu(), x) and torch.equal(b.pos.cpu(), pos) and torch.equal(b.edge_index.cpu(), ei)
            assert int(labels[g]) == lab
            seen += 1
    assert seen == 8


def test_superpixel_minibatches_run_eagerly_and_match_the_oracle_loop(tmp_path):
    from graphnet_classifier_amd.dataset import GraphImageFolder
    from graphnet_classifier_amd.train import train
    ds = GraphImageFolder(_folder(tmp_path / "data", side=48, smooth=True), resize_value=48, method="superpixel", n_segments=30)
    graphs = _cpu_graphs(ds)
    counts = [g[0][0].size(0) for g in graphs]
    print("superpixel node counts", counts)
    assert len(set(counts)) > 1 and min(counts) >= 2
    num_nodes = sorted(counts)[len(counts) // 2]  # some graphs smaller, some larger
    assert min(counts) < num_nodes or max(counts) > num_nodes
    m = _model(num_nodes, ragged=True)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    r = train(m, ds.loader(shuffle=False, batch_size=3), 1, patience=5, output_path=str(tmp_path / "run"))
    ref_loss, _ = _oracle_training(sd0, graphs, [[[0, 1, 2], [3, 4, 5], [6, 7, 8], [9]]], num_nodes)
    print("avg_loss", r["avg_loss"], "oracle", ref_loss)
    assert r["batched"] is True and r["captured"] is False
    assert abs(r["avg_loss"][0] - ref_loss[0]) <= 1e-5


@pytest.mark.parametrize("batch_size", [1, 4])
def test_evaluate_and_predict_agree_with_per_image_calls(tmp_path, batch_size):
    from graphnet_classifier_amd.dataset import GraphImageFolder
    from graphnet_classifier_amd.train import evaluate, predict
    ds = GraphImageFolder(_folder(tmp_path / "data"), resize_value=16, method="pixel")
    m = _model(256)
    with torch.no_grad():
        per_image = [(m(tuple(t.to(DEV) for t in g)), lab) for g, lab in _cpu_graphs(ds)]
    logits_ref = torch.stack([l for l, _ in per_image])
    labels = torch.tensor([lab for _, lab in per_image])
    pred = logits_ref.argmax(1).cpu()
    confusion = torch.zeros(2, 2, dtype=torch.int64)
    for a, b in zip(labels.tolist(), pred.tolist()):
        confusion[a, b] += 1
    loader = ds.loader(shuffle=False, batch_size=batch_size)
    ev = evaluate(m, loader)
    assert ev["count"] == 10 and ev["confusion"].dtype == torch.int64 and torch.equal(ev["confusion"], confusion)
    assert ev["accuracy"] == float((pred == labels).sum()) / 10
    ce = float(torch.nn.functional.cross_entropy(logits_ref.double().cpu(), labels))
    assert abs(ev["loss"] - ce) <= 1e-5
    logits, prob = predict(m, loader)
    assert logits.shape == prob.shape == (10, 2) and max_abs(logits, logits_ref) <= 1e-5  # loader order = dataset order
    assert max_abs(prob.sum(1), torch.ones(10, device=prob.device)) <= 1e-6
    assert max_abs(prob, torch.softmax(logits_ref, -1)) <= 1e-5
