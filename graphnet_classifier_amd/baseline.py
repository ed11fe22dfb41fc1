"""The image-MLP baseline the graph model is compared with: the reference's ``load_data`` / ``train_MLP`` (``main.py:13-29``) and
``mlp_inference`` (``utils/inference.py:16-29``) on the device path, without torchvision.

``train_MLP()`` trains ``MLP(3 * R * R, num_classes)`` on ``ImageFolder`` batches of 8: the folder is read by
``dataset.ImageTensorFolder`` (Pillow-exact BILINEAR resize and ``ToTensor`` on the device), the first Linear - 49152 inputs for 8
rows at the default size - runs on the split-K kernels K16, and the whole step is replayed from a hipGraph
(``train.CapturedTensorStep``).  ``mlp_inference`` scores one image file the way the reference does, quirks included: Pillow's
default (BICUBIC) resize BEFORE the conversion to RGB, and raw 0 ... 255 pixel values in H, W, C order - not what ``train_MLP``
feeds the model.
"""
from __future__ import annotations

import numpy as np
import torch

from . import image_to_graph as I2G
from .MLP import MLP
from .dataset import ImageTensorFolder
from .train import check_optimizer_options, make_criterion, train

TRAINING_CONTROLS = ("optimizer", "lr", "weight_decay", "momentum", "nesterov", "max_grad_norm", "lr_schedule", "skip_nonfinite")
LOSS_CONTROLS = ("loss", "class_weight", "label_smoothing", "pos_weight", "metrics")


def load_data(dataset_path, resize_value=128, batch_size=8):
    """``main.py:13-18``: shuffled mini-batches of ``(float32 [B, 3, R, R], labels [B])`` over an image folder; every iteration
    of the returned loader is one epoch.  ``loader.dataset.classes`` names the classes, as on the reference's ``DataLoader``."""
    return ImageTensorFolder(dataset_path, resize_value).loader(batch_size=batch_size, shuffle=True)


def train_MLP(epochs=30, channels=3, resize_value=128, batch_size=8, hidden_layers=2, output_path='weights/MLP', dataset_path='dataset',
              **training_controls):
    """``main.py:21-29`` (``dataset_path`` is one addition: the reference hard-codes ``'dataset'``; ``training_controls`` the other:
    ``train``'s ``optimizer``, ``weight_decay``, ``momentum``, ``nesterov``, ``max_grad_norm``, ``lr_schedule``, ``skip_nonfinite``
    and ``lr``, and its loss keywords ``loss``, ``class_weight``, ``label_smoothing``, ``pos_weight`` and ``metrics``, all checked
    before the folder is read).  Returns ``train``'s dict with the model under ``"model"``."""
    unknown = sorted(set(training_controls) - set(TRAINING_CONTROLS) - set(LOSS_CONTROLS))
    if unknown:
        raise ValueError(f"train_MLP: unknown training controls {unknown}; {TRAINING_CONTROLS + LOSS_CONTROLS} expected")
    check_optimizer_options(**{k: v for k, v in training_controls.items() if k != "skip_nonfinite" and k not in LOSS_CONTROLS})
    make_criterion(**{k: v for k, v in training_controls.items() if k in LOSS_CONTROLS})  # the check alone: train() makes its own
    loader = load_data(dataset_path, resize_value, batch_size)
    model = MLP(in_dim=channels * resize_value * resize_value, out_dim=len(loader.dataset.classes), hidden_layers=hidden_layers)
    history = train(model, loader, epochs, patience=5, output_path=output_path, **training_controls)
    history["model"] = model
    return history


def inference_pixels(image_path, resize_value=128) -> torch.Tensor:
    """The uint8 ``[R, R, 3]`` array ``np.array(Image.open(path).resize((R, R)).convert('RGB'))`` on the device.  An image that is
    already RGB is resized by the device kernel (byte for byte Pillow's BICUBIC); any other mode is resized in its own mode by
    Pillow on the host, as the reference's order of operations asks, and converted afterwards."""
    from PIL import Image
    with Image.open(image_path) as img:
        if img.mode == "RGB":
            return I2G.resize(np.array(img), (resize_value, resize_value), "bicubic")
        pixels = np.array(img.resize((resize_value, resize_value)).convert("RGB"))
    return torch.from_numpy(pixels).to(I2G._device())


def mlp_inference(image_path, weights='weights/MLP/final_model_.pth', resize_value=128):
    """``utils/inference.py:16-29``: ``(logits [1, 2], softmax [1, 2])`` of ``MLP(3 * R * R, 2)`` with the state dict at
    ``weights`` on one image file.  The input is the raw 0 ... 255 pixel values flattened in H, W, C order."""
    model = MLP(in_dim=resize_value * resize_value * 3, out_dim=2)
    model.load_state_dict(torch.load(weights, map_location="cpu"))
    model.eval()
    with torch.no_grad():
        pixels = inference_pixels(image_path, resize_value)
        logits = model(pixels.flatten().to(torch.float32).unsqueeze(0))
        return logits, torch.softmax(logits, dim=1)
