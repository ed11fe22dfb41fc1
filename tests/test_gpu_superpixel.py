"""GPU: the device SLIC (csrc/superpixel.hip) against scikit-image 0.18.3 and the reference's superpixel graphs
(tests/golden/g10_superpixel*.npz): labels bit for bit, graphs, batching, degenerate inputs, a model forward."""
import numpy as np
import pytest
import torch

from oracle import graphnet_oracle as O
from tests._util import max_abs
from tests.test_superpixel_golden import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def I2G():
    from graphnet_classifier_amd import image_to_graph
    return image_to_graph


def _slic(I2G, img, params, **kw):
    n, c, mi, ec = params
    return I2G.slic(img, n_segments=n, compactness=c, max_iter=mi, enforce_connectivity=ec, return_counts=True, **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"case{c[0]}-{c[1].shape[0]}x{c[1].shape[1]}-{c[3]}")
def test_slic_labels_match_scikit_image_bit_for_bit(I2G, case):
    _, img, ref, params, _ = case
    labels, counts = _slic(I2G, img, params)
    got = labels.cpu().numpy()
    assert labels.dtype == torch.int32 and labels.is_cuda and got.shape == ref.shape
    mism = int((got != ref).sum())
    assert mism == 0, f"{mism} of {ref.size} pixels differ"
    if params[3]:
        assert int(counts[0]) == len(np.unique(ref)) == int(ref.max()) + 1
    else:
        assert int(counts[0]) > int(ref.max())  # the number of grid centres


@pytest.mark.parametrize("case", [c for c in CASES if c[4] is not None], ids=lambda c: f"case{c[0]}")
def test_superpixel_graph_from_array_matches_reference(I2G, case):
    _, img, labels, _, (rx, rpos, rei) = case
    for x, pos, ei in (I2G.superpixel_graph_from_array(img), I2G.superpixel_graph_from_labels(img, labels)):
        assert ei.dtype == torch.int64 and np.array_equal(ei.cpu().numpy(), rei)
        assert x.shape == rx.shape and float(np.abs(x.cpu().numpy() - rx).max()) <= 1e-6
        assert pos.shape == rpos.shape and float(np.abs(pos.cpu().numpy() - rpos).max()) <= 1e-6


def test_image_to_graph_superpixel_runs_on_the_device(I2G):
    from PIL import Image
    _, img, _, _, (rx, rpos, rei) = next(c for c in CASES if c[1].shape == (64, 64, 3) and c[4] is not None)
    x, pos, ei = I2G.image_to_graph_superpixel(Image.fromarray(img), resize_value=64)
    assert x.is_cuda and np.array_equal(ei.cpu().numpy(), rei)
    assert float(np.abs(x.cpu().numpy() - rx).max()) <= 1e-6
    with pytest.raises(NotImplementedError):
        I2G.image_to_graph_superpixel(Image.fromarray(img), resize_value=64, sigma=1.0)


def test_batch_equals_per_image(I2G):
    imgs = [c for c in CASES if c[1].shape == (64, 64, 3)]
    batch = np.stack([imgs[i % len(imgs)][1] for i in range(24)])
    batch[8:] = np.roll(batch[8:], 3, axis=2)  # more than the fixture's distinct images
    batch[16:] = batch[16:, ::-1]
    labels, counts = I2G.slic(batch, return_counts=True)
    assert labels.shape == (24, 64, 64) and counts.shape == (24,)
    for i in range(24):
        li, ci = I2G.slic(batch[i], return_counts=True)
        assert torch.equal(li, labels[i]) and int(ci[0]) == int(counts[i])
    for _, img, ref, params, _ in imgs[:8]:
        if params == (100, 10.0, 10, True):
            k = next(i for i in range(8) if np.array_equal(batch[i], img))
            assert np.array_equal(labels[k].cpu().numpy(), ref)


def _components_are_single_regions(lab):
    from scipy import ndimage
    for v in np.unique(lab):
        _, n = ndimage.label(lab == v)  # 4-connectivity
        if n != 1:
            return False
    return True


@pytest.mark.parametrize("shape,n_segments", [((17, 23), 10), ((1, 1), 1), ((1, 40), 5), ((40, 1), 7), ((9, 7), 1),
                                              ((9, 7), 63), ((6, 5), 30), ((33, 48), 100)])
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ramp"])
@pytest.mark.parametrize("start_label", [0, 1])
def test_degenerate_inputs(I2G, shape, n_segments, uniform, start_label):
    yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    ramp = np.stack([yy * 255 // max(shape[0] - 1, 1), xx * 255 // max(shape[1] - 1, 1), np.full(shape, 128)], -1)
    img = np.full(shape + (3,), 128, np.uint8) if uniform else ramp.astype(np.uint8)
    for ec in (True, False):
        labels, counts = I2G.slic(img, n_segments=n_segments, enforce_connectivity=ec, start_label=start_label,
                                  return_counts=True)
        lab, cnt = labels.cpu().numpy(), int(counts[0])
        assert lab.shape == shape and cnt >= 1
        assert lab.min() >= start_label and lab.max() < start_label + cnt
        if ec:
            assert _components_are_single_regions(lab)


def test_unsupported_options_raise(I2G):
    img = np.zeros((8, 8, 3), np.uint8)
    from graphnet_classifier_amd import native
    for kw in (dict(start_label=2), dict(compactness=0), dict(max_iter=0)):
        with pytest.raises(RuntimeError, match="gnc_slic_rgb_u8"):
            I2G.slic(img, **kw)
    assert native.load_library().gnc_slic_workspace_bytes(1, 8, 8, 0) == 0


def test_graphnet_forward_on_device_superpixel_graph(I2G):
    from graphnet_classifier_amd.GNN import GraphNet
    torch.manual_seed(0)
    m = GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3).cuda()  # main.py:72
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for _, img, _, _, (rx, rpos, rei) in [c for c in CASES if c[4] is not None][::5]:
        x, pos, ei = I2G.superpixel_graph_from_array(img)
        with torch.no_grad():
            y = m(x, pos, ei).cpu()
        ref = O.graphnet_forward(sd, torch.from_numpy(rx), torch.from_numpy(rpos), torch.from_numpy(rei))
        assert max_abs(y, ref) < 1e-5
