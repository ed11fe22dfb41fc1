"""GPU, end to end: ``GraphImageFolder(method='superpixel')`` -> ``train()`` on graphs whose node counts differ from image
to image (SLIC hands out another number of segments per photo), eagerly and through the node-capacity capture."""
import ast
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests._util import load_golden, sub_state_dict
from tests.test_superpixel_golden import CASES

pytestmark = pytest.mark.gpu


def test_superpixel_folder_trains_eagerly_and_captured(tmp_path):
    """The eight 64 x 64 fixture photos (87 to 119 segments at the default parameters, five above ``num_nodes`` = 100):
    the captured run - one hipGraph over a node and an edge capacity - gives the eager run's losses and weights."""
    from graphnet_classifier_amd.dataset import GraphImageFolder
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    from graphnet_classifier_amd.train import train
    root = tmp_path / "photos"
    for k, case_id in enumerate(range(8, 16)):
        cid, img, _, _, _ = CASES[case_id]
        assert cid == case_id and img.shape == (64, 64, 3)
        cls = root / ("even" if k % 2 == 0 else "odd")
        os.makedirs(cls, exist_ok=True)
        Image.fromarray(img).save(cls / f"photo{k}.png")
    ds = GraphImageFolder(str(root), resize_value=64, method="superpixel")
    counts = [int(g[0].size(0)) for g, _ in ds.loader(shuffle=False)]
    assert len(counts) == 8 and len(set(counts)) >= 3 and max(counts) > 100 > min(counts)

    g = load_golden("g8_training_run.npz")
    kw = ast.literal_eval(bytes(g["kwargs_json"]).decode())
    gsd = {k[len("graph_net."):]: v for k, v in sub_state_dict(g, "before/").items() if k.startswith("graph_net.")}
    out = {}
    for capture in (False, True):
        torch.manual_seed(99)
        m = CombinedModel(GraphNet(**kw), num_nodes=100, classes=2)
        m.graph_net.load_state_dict(gsd, strict=True)
        m.ragged_readout = True
        r = train(m, ds.loader(shuffle=False), 3, patience=5, output_path=str(tmp_path / str(capture)), capture=capture)
        assert r["captured_ragged"] is capture
        assert len(r["avg_loss"]) == 3 and all(np.isfinite(v) for v in r["avg_loss"])
        out[capture] = ({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, r["avg_loss"])
    print("avg_loss eager", out[False][1], "captured", out[True][1])
    for a, b in zip(out[True][1], out[False][1]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (out[True][1], out[False][1])
    close = total = 0
    for k in out[True][0]:
        d = (out[True][0][k] - out[False][0][k]).abs()
        close += int((d <= 2e-5).sum())
        total += d.numel()
    print(f"weights within 2e-5: {close} of {total}")
    # an entry whose gradient is at rounding level moves by ~lr per step in a direction fp32 noise decides (as in G8)
    assert close >= 0.97 * total, (close, total)
