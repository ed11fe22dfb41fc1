"""GPU: the training controls of ``train()`` (DESIGN K22) end to end on the golden inputs of tests/golden/g8_training_run.npz (64
nodes, two samples): AdamW and SGD with clipping and a warm-up + cosine schedule, the captured run against the eager one bit for
bit, the per-epoch history, the defaults spelled out, and a ``CapturedRaggedBatchStep`` that steps ``FusedSGD``."""
import ast

import numpy as np
import pytest
import torch

from tests import optimizer_control_cases as C
from tests._util import load_golden, max_abs, sub_state_dict, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPOCHS = 3  # two samples each: six optimizer steps
SCHEDULE = dict(kind="cosine", warmup_steps=2, total_steps=6, min_lr=1e-5)
CONTROLS = {
    "adamw": dict(optimizer="adamw", lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, lr_schedule=SCHEDULE),
    "sgd": dict(optimizer="sgd", lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4, max_grad_norm=1.0, lr_schedule=SCHEDULE),
}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g8_training_run.npz")


def _dataset(g):
    pos, ei = t(g["pos"]), t(g["edge_index"])
    xs = [t(g["x0"]), t(g["x1"])]
    return [((xs[k], pos, ei), torch.tensor(int(g["labels"][k]))) for k in range(2)]


def _run(g, out, **kw):
    from graphnet_classifier_amd import GNN
    from graphnet_classifier_amd.train import train
    m = GNN.CombinedModel(GNN.GraphNet(**ast.literal_eval(bytes(g["kwargs_json"]).decode())), num_nodes=64, classes=2)
    m.load_state_dict(sub_state_dict(g, "before/"), strict=True)
    r = train(m, _dataset(g), EPOCHS, patience=5, output_path=str(out), **kw)
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, r


def _within_one_ulp(got, want) -> bool:
    return abs(float(got) - float(np.float32(want))) <= float(np.spacing(np.float32(want)))


@pytest.mark.parametrize("name", list(CONTROLS))
def test_captured_training_equals_eager_training_under_the_controls(golden, tmp_path, name):
    kw = CONTROLS[name]
    runs = {capture: _run(golden, tmp_path / str(capture), capture=capture, **kw) for capture in (False, True)}
    for capture, (weights, r) in runs.items():
        assert r["captured"] == capture and r["skipped_steps"] == 0 and int(r["optimizer"].step_count.item()) == 2 * EPOCHS
        assert len(r["lr"]) == len(r["grad_norm"]) == len(r["avg_loss"]) == EPOCHS
        for epoch, lr in enumerate(r["lr"], start=1):  # of each epoch's last step
            assert _within_one_ulp(lr, C.lr_at(2 * epoch, kw["lr"], **SCHEDULE)), (epoch, lr)
        assert r["lr"][-1] == float(np.float32(1e-5)) and all(np.isfinite(n) and n > 0 for n in r["grad_norm"])
        assert all(torch.isfinite(v).all() for v in weights.values())
    print(name, "lr", runs[True][1]["lr"], "grad_norm", runs[True][1]["grad_norm"], "avg_loss", runs[True][1]["avg_loss"])
    assert runs[True][1]["avg_loss"] == runs[False][1]["avg_loss"] and runs[True][1]["grad_norm"] == runs[False][1]["grad_norm"]
    for k, v in runs[True][0].items():
        assert torch.equal(v, runs[False][0][k]), k
    before = sub_state_dict(golden, "before/")
    assert any(not torch.equal(v, before[k]) for k, v in runs[True][0].items())  # it trained


def test_the_defaults_spelled_out_are_the_defaults(golden, tmp_path):
    plain, r0 = _run(golden, tmp_path / "plain")
    spelled, r1 = _run(golden, tmp_path / "spelled", optimizer="adam", lr=1e-3, weight_decay=0.0, momentum=0.0, nesterov=False,
                       max_grad_norm=None, lr_schedule=None, skip_nonfinite=False)
    assert r0["avg_loss"] == r1["avg_loss"] and not r1["optimizer"].controlled
    for k, v in plain.items():
        assert torch.equal(v, spelled[k]), k
    assert r1["lr"] == [float(np.float32(1e-3))] * EPOCHS and r1["skipped_steps"] == 0 and all(np.isnan(n) for n in r1["grad_norm"])


def test_a_ragged_batch_capture_steps_fused_sgd():
    """Two padded batches through one ``CapturedRaggedBatchStep`` against two eager steps.  The captured gradients agree with the
    eager ones to 2e-5 + 1e-4 max|g| (tests/test_gpu_ragged_batch_capture.py); two steps at lr 1e-2 with |clip_coef| <= 1 and
    momentum 0.9 move a parameter by at most (1 + 1.9) lr times that: 1e-5 leaves room for max|g| up to 3."""
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    from graphnet_classifier_amd.train import CapturedRaggedBatchStep, FlatParameters, FusedSGD, lr_at

    def model():
        torch.manual_seed(99)
        m = CombinedModel(GraphNet(**synthetic.graphnet_kwargs(32, 1)), num_nodes=12, classes=2)
        m.ragged_readout = True
        return m

    shapes = ((3, 3), (3, 4), (4, 4))
    batches = [synthetic.superpixel_like_graphs(3, seed, shapes=shapes) for seed in (208, 207)]  # 48 nodes, then 27
    labels = [torch.tensor([0, 1, 1]), torch.tensor([1, 0, 1])]
    sched = dict(kind="step", warmup_steps=1, gamma=0.5, every=1)
    kw = dict(momentum=0.9, weight_decay=1e-4, max_grad_norm=5.0, lr_schedule=sched)
    crit = torch.nn.CrossEntropyLoss()
    e = model()
    eopt = FusedSGD(FlatParameters(e), 1e-2, **kw)
    for b, y in zip(batches, labels):
        loss = crit(e.forward_batched(b.x.to(DEV), b.pos.to(DEV), b.edge_index.to(DEV), graph_ptr=b.graph_ptr), y.to(DEV))
        eopt.zero_grad()
        loss.backward()
        eopt.step()
    m = model()
    opt = FusedSGD(FlatParameters(m), 1e-2, **kw)
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    step = CapturedRaggedBatchStep(m, opt, crit, batches[0].to(DEV), labels[0], loss_sum, edge_capacity=256, node_capacity=64)
    assert int(opt.step_count.item()) == 0 and float(loss_sum.item()) == 0.0 and not bool(opt.momentum_buffer.any())
    assert np.isnan(float(opt.grad_norm)) and int(opt.skipped_steps) == 0  # the warm-up steps are undone, the new state included
    for b, y in zip(batches, labels):
        step(b.to(DEV), y)
    step.check()
    torch.cuda.synchronize()
    assert int(opt.step_count.item()) == int(eopt.step_count.item()) == 2 and int(opt.skipped_steps) == int(eopt.skipped_steps) == 0
    assert float(opt.current_lr) == float(eopt.current_lr) == float(np.float32(lr_at(2, 1e-2, **sched))) == float(np.float32(0.5e-2))
    norm, want = float(opt.grad_norm), float(eopt.grad_norm)
    err = max_abs(opt.fp.flat, eopt.fp.flat)
    print(f"grad_norm captured {norm!r} eager {want!r}; max |p captured - p eager| = {err:.3e}; max |g| = {float(eopt.fp.grad.abs().max()):.3e}")
    assert np.isfinite(norm) and norm > 0 and float(eopt.fp.grad.abs().max()) <= 3.0
    assert err <= 1e-5 and bool(torch.isfinite(opt.fp.flat).all())
