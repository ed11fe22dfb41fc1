#!/usr/bin/env python3
"""Capture tests/golden/g12_image_mlp.npz by running the REFERENCE's own ``MLP`` (models/MLP.py) and ``train()``
(utils/train_model.py) on a tiny image folder, the way its ``train_MLP`` does (main.py:21-29; ``main.py`` itself needs torchvision
and is not imported).

Run in the build container only (needs /root/reference):

    python tests/golden/make_image_mlp_golden.py

The file holds data only: 19 small synthetic photos (uint8 arrays, two classes; the tests write them out as PNG files), what
``transforms.Resize((20, 20))`` makes of them (Pillow BILINEAR on the PIL image), the seeds of the model and of the loader, and what the
reference computed: the average loss of each of 3 epochs at ``batch_size=8`` (two full batches and a short one per epoch), the sample
indices and logits of the first batch, and the first step's gradients of every tensor except the first Linear's weight.  It holds no
weight matrix: ``MLP(1200, 2)`` under ``torch.manual_seed(MODEL_SEED)`` is the model.

The same three epochs are also run in float64 (the reference's modules cast up, torch.optim.Adam, the same batches) and stored as
``epoch_losses_float64``: the distance between the two runs (4e-7) is what fp32 rounding does to this run, far below the 1e-5 the
tests hold train() to.
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch
from PIL import Image

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
MODEL_SEED, LOADER_SEED, EPOCHS, BATCH, SIDE = 3, 11, 3, 8, 20


def photo(h, w, seed):
    """smooth colour fields with some noise (the fixture photos of tests/test_gpu_image_folder.py)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [127 + 120 * np.sin(xx / rng.uniform(5, 40) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(5, 40)) for _ in range(3)]
    return np.clip(np.stack(chans, -1) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def main():
    sys.path.insert(0, REF)
    from models.MLP import MLP
    from utils.train_model import train

    sizes = [(30, 40), (48, 36), (25, 25), (64, 50), (20, 20), (33, 57), (41, 29), (52, 52), (19, 23), (36, 48),
             (28, 61), (45, 45), (60, 32), (22, 38), (39, 39), (50, 27), (31, 31), (44, 58), (27, 49)]
    photos = [photo(h, w, 100 + i) for i, (h, w) in enumerate(sizes)]
    labels = np.array([0] * 10 + [1] * 9, dtype=np.int64)  # ImageFolder order: class 0's files, then class 1's
    resized = np.stack([np.array(Image.fromarray(p).resize((SIDE, SIDE), Image.Resampling.BILINEAR)) for p in photos])
    samples = [(torch.from_numpy(r).permute(2, 0, 1).float().div(255), int(l)) for r, l in zip(resized, labels)]  # ToTensor

    def reference_run(model_seed):
        torch.manual_seed(model_seed)
        model = MLP(in_dim=3 * SIDE * SIDE, out_dim=2)
        step_logits, step_labels, first_grads = [], [], {}

        class Recorded(torch.utils.data.DataLoader):  # the labels of every step, in step order
            def __iter__(self):
                for x, y in super().__iter__():
                    step_labels.append(y.clone())
                    yield x, y

        model.register_forward_hook(lambda mod, args, out: step_logits.append(out.detach().clone()))
        def record(name):
            def hook(grad):  # returns None: the gradient stays as it is
                first_grads.setdefault(name, grad.detach().clone())
            return hook

        for n, p in model.named_parameters():
            p.register_hook(record(n))
        torch.manual_seed(LOADER_SEED)
        loader = Recorded(samples, batch_size=BATCH, shuffle=True)
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
            train(model, loader, EPOCHS, patience=5, output_path=tmp)
        criterion = torch.nn.CrossEntropyLoss()
        losses = [float(criterion(lg, lb)) for lg, lb in zip(step_logits, step_labels)]
        per_epoch = len(losses) // EPOCHS
        epoch_losses = np.array([sum(losses[e * per_epoch:(e + 1) * per_epoch]) / per_epoch for e in range(EPOCHS)], dtype=np.float64)
        return [n for n, _ in model.named_parameters()], step_logits, step_labels, first_grads, losses, epoch_losses

    def float64_run(model_seed):
        torch.manual_seed(model_seed)
        model = MLP(in_dim=3 * SIDE * SIDE, out_dim=2).double()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        x = torch.stack([s for s, _ in samples]).double().reshape(len(samples), -1)
        y = torch.from_numpy(labels)
        torch.manual_seed(LOADER_SEED)
        loader = torch.utils.data.DataLoader(list(range(len(samples))), batch_size=BATCH, shuffle=True)
        out = []
        for _ in range(EPOCHS):
            total, steps = 0.0, 0
            for idx in loader:
                loss = torch.nn.functional.cross_entropy(model.model(x[idx]), y[idx])
                opt.zero_grad()
                loss.backward()
                opt.step()
                total, steps = total + float(loss), steps + 1
            out.append(total / steps)
        return np.array(out)

    names, step_logits, step_labels, first_grads, losses, epoch_losses = reference_run(MODEL_SEED)
    f64_losses = float64_run(MODEL_SEED)
    print("float32 / float64 epoch losses differ by", float(np.abs(epoch_losses - f64_losses).max()))
    # the first batch's sample indices: the loader's order under LOADER_SEED, re-drawn
    torch.manual_seed(LOADER_SEED)
    first_idx = next(iter(torch.utils.data.DataLoader(list(range(len(samples))), batch_size=BATCH, shuffle=True))).numpy()
    arrays = {f"photo_{i:02d}": p for i, p in enumerate(photos)}
    arrays.update({"grad/" + n: first_grads[n].numpy() for n in names if n != "model.0.weight"})
    np.savez_compressed(os.path.join(OUT, "g12_image_mlp.npz"), labels=labels, resized=resized, model_seed=np.array(MODEL_SEED),
                        loader_seed=np.array(LOADER_SEED), epochs=np.array(EPOCHS), batch_size=np.array(BATCH), side=np.array(SIDE),
                        epoch_losses=epoch_losses, epoch_losses_float64=f64_losses, step_losses=np.array(losses, dtype=np.float64), first_batch_indices=first_idx,
                        first_batch_labels=step_labels[0].numpy(), first_batch_logits=step_logits[0].numpy(), **arrays)
    print("g12_image_mlp.npz:", epoch_losses, first_idx, os.path.getsize(os.path.join(OUT, "g12_image_mlp.npz")), "bytes")


if __name__ == "__main__":
    main()
