"""Image-folder training data without torchvision: the reference's ``utils/dataloader.py`` (``OptimizedDatasetLoader``
over ``torchvision.datasets.ImageFolder``) on the device path.

``GraphImageFolder(dataset_path, resize_value, diagonals, method, n_segments, patch_size, use_cache)`` finds images
by torchvision's ``ImageFolder`` rules and yields ``((x, pos, edge_index), label)`` as the reference's
``__getitem__`` does, with the tensors already on the GPU.  It is a ``torch.utils.data.Dataset``, so ``main.py``'s
``DataLoader(ds, batch_size=1, shuffle=True, collate_fn=lambda b: b[0])`` works unchanged.  Behind the reference's own
parameters, ``edges="knn"`` (with ``knn_k`` and ``knn_pos_weight``) swaps a method's edge list for the k nearest neighbours of
every node in (colour, position), ``image_to_graph.graphs_from_images``' option (DESIGN K24); ``edges=None`` is the reference.
``node_features="descriptor"`` (superpixel only, DESIGN K26) widens ``x`` from the mean colour to 16 region descriptor columns;
``num_node_features`` is the width to build the model with.

``GraphImageFolder.loader()`` is the fast way through an epoch: the same samples in the same order as that
``DataLoader`` (and the same draws from the global RNG), with decoding on a host thread pool and the resize and the
graph builds of a chunk of images run as batched launches (``image_to_graph.graphs_from_images``).

``ImageTensorFolder(dataset_path, resize_value)`` is the image side of the reference's MLP baseline (``main.py:13-18``:
``ImageFolder`` + ``Resize`` + ``ToTensor``): ``(float32 [3, R, R], label)`` per image, and ``.loader(batch_size=8)`` yields the
mini-batches of ``DataLoader(ds, batch_size=8, shuffle=True)`` as ``(float32 [B, 3, R, R] on the device, labels [B])``.

Both folders take ``augment=augment.Augmentation(...)`` (K25): their loaders then crop, flip and colour-jitter every image anew in
every epoch, on the device and with Pillow's pixels, from parameters keyed by ``(seed, epoch, sample index)``.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from torch.utils.data import Dataset

from . import image_to_graph as I2G

# torchvision.datasets.folder.IMG_EXTENSIONS
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
MAX_WORKERS = 16


def find_classes(directory: str):
    """Sorted sub-directory names and their indices (torchvision ``find_classes``)."""
    classes = sorted(entry.name for entry in os.scandir(directory) if entry.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {directory}.")
    return classes, {name: i for i, name in enumerate(classes)}


def make_dataset(directory: str, class_to_idx, extensions=IMG_EXTENSIONS):
    """``(path, class_index)`` pairs in torchvision ``make_dataset`` order: classes sorted, then
    ``sorted(os.walk(class_dir, followlinks=True))`` with sorted file names, extensions matched case-insensitively.
    A class without images raises ``FileNotFoundError``."""
    directory = os.path.expanduser(directory)
    instances, empty = [], []
    for target_class in sorted(class_to_idx):
        class_index = class_to_idx[target_class]
        target_dir = os.path.join(directory, target_class)
        if not os.path.isdir(target_dir):
            continue
        found = False
        for root, _, fnames in sorted(os.walk(target_dir, followlinks=True)):
            for fname in sorted(fnames):
                path = os.path.join(root, fname)
                if path.lower().endswith(extensions):
                    instances.append((path, class_index))
                    found = True
        if not found:
            empty.append(target_class)
    if empty:
        raise FileNotFoundError(f"Found no valid file for the classes {', '.join(sorted(empty))}. "
                                f"Supported extensions are: {', '.join(extensions)}")
    return instances


def load_rgb(path: str) -> np.ndarray:
    """torchvision's ``pil_loader``: ``Image.open(f).convert("RGB")``, as a uint8 [H, W, 3] array."""
    from PIL import Image
    with open(path, "rb") as f:
        img = Image.open(f)
        return np.array(img.convert("RGB"))


def _check_augment(augment):
    from .augment import Augmentation
    if augment is not None and not isinstance(augment, Augmentation):
        raise TypeError(f"augment must be an augment.Augmentation or None, got {type(augment).__name__}")
    return augment


def default_workers() -> int:
    """``OMP_NUM_THREADS`` capped at 16 (never the machine's CPU count: a job is given a share of it)."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", ""))
    except ValueError:
        n = 0
    return max(1, min(n if n > 0 else MAX_WORKERS, MAX_WORKERS))


class GraphImageFolder(Dataset):
    """``utils/dataloader.py``'s ``OptimizedDatasetLoader`` (same parameters and defaults) over an image folder laid
    out as ``torchvision.datasets.ImageFolder`` expects (``root/<class>/.../<image>``)."""

    def __init__(self, dataset_path='dataset', resize_value=128, diagonals=False, method='pixel', n_segments=100,
                 patch_size=8, use_cache=True, edges=None, knn_k=8, knn_pos_weight=1.0, augment=None, node_features=None):
        if method not in I2G.METHODS:
            raise ValueError(f"Unknown method: {method}")
        I2G.check_edges(edges, knn_k)
        I2G.check_node_features(node_features, method)
        self.dataset_path = dataset_path
        self.classes, self.class_to_idx = find_classes(dataset_path)
        self.samples = make_dataset(dataset_path, self.class_to_idx)
        self.targets = [t for _, t in self.samples]
        self.resize_value = resize_value
        self.diagonals = diagonals
        self.method = method
        self.n_segments = n_segments
        self.patch_size = patch_size
        self.use_cache = use_cache
        self.edges = edges  # None: the method's own edges; "knn": k nearest neighbours in (colour, position) (K24)
        self.knn_k = knn_k
        self.knn_pos_weight = knn_pos_weight
        self.augment = _check_augment(augment)  # an augment.Augmentation for the loaders (K25); None: the plain images
        self.node_features = node_features  # None: the method's own x; "descriptor": 16 region descriptor columns (superpixel, K26)

    def __len__(self):
        return len(self.samples)

    @property
    def num_node_features(self) -> int:
        """Columns of ``x``, for ``GraphNet(num_local_features=...)``: 3, or 16 under ``node_features="descriptor"``."""
        return 3 if self.node_features is None else I2G.REGION_DESCRIPTOR_DIM

    def _graphs(self, images, augmentation=None):
        return I2G.graphs_from_images(images, self.method, resize_value=self.resize_value, diagonals=self.diagonals,
                                      use_cache=self.use_cache, n_segments=self.n_segments,
                                      patch_size=self.patch_size, edges=self.edges, knn_k=self.knn_k,
                                      knn_pos_weight=self.knn_pos_weight, augmentation=augmentation,
                                      node_features=self.node_features)

    _build = _graphs  # what a loader calls per chunk

    def __getitem__(self, idx):
        """The plain, un-augmented graph of image ``idx`` whatever ``augment`` is: augmentation belongs to an epoch, and only the
        loaders know which one is running."""
        path, label = self.samples[idx]
        return self._graphs([load_rgb(path)])[0], torch.tensor(label, dtype=torch.long)

    def loader(self, shuffle: bool = True, chunk: int = 64, workers: int | None = None, batch_size: int = 1,
               drop_last: bool = False, augment: bool = True):
        """Iterable for ``train(model, ds.loader(), epochs, ...)``; every iteration is one epoch.

        ``batch_size=1``: ``((x, pos, edge_index), label)`` per image, in the order ``DataLoader(self, batch_size=1,
        shuffle=shuffle)`` would give under the same global RNG state.  ``batch_size=B > 1``: ``(GraphBatch, labels [B])``
        per mini-batch (``image_to_graph.collate_graphs``), the batches being those of ``DataLoader(self, batch_size=B,
        shuffle=shuffle, drop_last=drop_last)`` under the same global RNG state; without ``drop_last`` the last batch
        may be shorter.

        ``augment=True`` applies the dataset's ``Augmentation`` (if it has one): every ``__iter__`` is one epoch with its own
        crops, flips and jitter, and advances the loader's epoch counter (``set_epoch(e)`` sets it).  ``augment=False`` gives the
        plain images of the same folder, for ``evaluate`` / ``predict``.  The order of the samples is the same either way."""
        return GraphFolderLoader(self, shuffle, chunk, workers, batch_size, drop_last, augment)


class GraphFolderLoader:
    """Epochs over a ``GraphImageFolder``: decode on a thread pool (the next chunk's decode is in flight while the
    current chunk is consumed), then resize and graph builds per chunk in batched launches."""

    def __init__(self, dataset: GraphImageFolder, shuffle: bool = True, chunk: int = 64, workers: int | None = None,
                 batch_size: int = 1, drop_last: bool = False, augment: bool = True):
        if chunk < 1:
            raise ValueError("chunk must be at least 1")
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.dataset = dataset
        self.shuffle = shuffle
        self.chunk = int(chunk)
        self.batch_size = int(batch_size)
        self.drop_last = bool(drop_last)
        self.workers = default_workers() if workers is None else max(1, min(int(workers), MAX_WORKERS))
        self.augment = getattr(dataset, "augment", None) if augment else None
        self.epoch = 0  # the epoch the next __iter__ runs; part of the key of every augmentation draw

    def set_epoch(self, epoch: int) -> None:
        """The epoch number of the next ``__iter__`` (each ``__iter__`` then counts on from it)."""
        self.epoch = int(epoch)

    def _next_epoch(self) -> int:
        epoch = self.epoch
        self.epoch = epoch + 1
        return epoch

    def _build(self, images, idx, epoch):
        """graphs (or tensors) of one decoded chunk, augmented with the parameters of samples ``idx`` in ``epoch``"""
        if self.augment is None:
            return self.dataset._build(images)
        params = self.augment.sample([im.shape[:2] for im in images], epoch, idx)
        return self.dataset._build(images, augmentation=params)

    def __len__(self):
        n, b = len(self.dataset), self.batch_size
        return n // b if self.drop_last else (n + b - 1) // b

    def order(self):
        """The epoch's sample indices, drawing from the global RNG exactly as a single-process ``DataLoader`` does:
        its iterator's base seed, then (shuffle only) ``RandomSampler``'s seed for a private generator."""
        torch.empty((), dtype=torch.int64).random_()  # _BaseDataLoaderIter._base_seed
        n = len(self.dataset)
        if not self.shuffle:
            return list(range(n))
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        generator = torch.Generator()
        generator.manual_seed(seed)
        return torch.randperm(n, generator=generator).tolist()

    def index_batches(self):
        """The epoch's index batches (host only): ``order()`` cut as ``BatchSampler(batch_size, drop_last)`` cuts it, so
        the same lists, and the same draws from the global RNG, as ``DataLoader(dataset, batch_size=batch_size,
        shuffle=shuffle, drop_last=drop_last)``."""
        order, b = self.order(), self.batch_size
        batches = [order[i:i + b] for i in range(0, len(order), b)]
        if self.drop_last and batches and len(batches[-1]) < b:
            batches.pop()
        return batches

    def __iter__(self):
        samples = self.dataset.samples
        epoch = self._next_epoch()
        if self.batch_size == 1:
            batches = None
            order = self.order()
            chunks = [order[i:i + self.chunk] for i in range(0, len(order), self.chunk)]
        else:  # a chunk holds whole mini-batches
            batches = self.index_batches()
            per = max(1, self.chunk // self.batch_size)
            groups = [batches[i:i + per] for i in range(0, len(batches), per)]
            chunks = [[i for b in group for i in b] for group in groups]
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            def decode(idx):
                return [pool.submit(load_rgb, samples[i][0]) for i in idx]

            pending = decode(chunks[0]) if chunks else []
            for c, idx in enumerate(chunks):
                images = [f.result() for f in pending]
                pending = decode(chunks[c + 1]) if c + 1 < len(chunks) else []
                graphs = self._build(images, idx, epoch)
                del images
                if batches is None:
                    for i, g in zip(idx, graphs):
                        yield g, torch.tensor(samples[i][1], dtype=torch.long)
                    continue
                at = 0
                for b in groups[c]:
                    yield (I2G.collate_graphs(graphs[at:at + len(b)]),
                           torch.tensor([samples[i][1] for i in b], dtype=torch.long))
                    at += len(b)


class ImageTensorFolder(Dataset):
    """``ImageFolder(root, transform=Compose([Resize((R, R)), ToTensor()]))`` of the reference's ``main.py:13-17`` without
    torchvision: the same classes, samples and order, the same pixel values (Pillow's BILINEAR resize and the division by 255
    run on the device, ``image_to_graph.tensors_from_images``)."""

    def __init__(self, dataset_path='dataset', resize_value=128, augment=None):
        self.dataset_path = dataset_path
        self.classes, self.class_to_idx = find_classes(dataset_path)
        self.samples = make_dataset(dataset_path, self.class_to_idx)
        self.targets = [t for _, t in self.samples]
        self.resize_value = resize_value
        self.augment = _check_augment(augment)  # an augment.Augmentation for the loader (K25); None: the plain images

    def __len__(self):
        return len(self.samples)

    def _build(self, images, augmentation=None):
        return I2G.tensors_from_images(images, self.resize_value, augmentation=augmentation)

    def __getitem__(self, idx):
        """The plain, un-augmented tensor of image ``idx`` whatever ``augment`` is (see ``GraphImageFolder.__getitem__``)."""
        path, label = self.samples[idx]
        return I2G.tensors_from_images([load_rgb(path)], self.resize_value)[0], label

    def loader(self, batch_size: int = 8, shuffle: bool = True, drop_last: bool = False, chunk: int = 64, workers: int | None = None,
               augment: bool = True):
        """Iterable for ``train(mlp, ds.loader(), epochs)``; every iteration is one epoch of ``(images float32 [B, 3, R, R] on the
        device, labels int64 [B])``, the batches being those of ``DataLoader(self, batch_size=batch_size, shuffle=shuffle,
        drop_last=drop_last)`` under the same global RNG state; without ``drop_last`` the last batch may be shorter.  ``augment`` as in
        ``GraphImageFolder.loader``: True applies the dataset's ``Augmentation``, anew in every epoch; False gives the plain images."""
        return TensorFolderLoader(self, shuffle, chunk, workers, batch_size, drop_last, augment)


class TensorFolderLoader(GraphFolderLoader):
    """Epochs over an ``ImageTensorFolder``: the index batches and the decode pipeline of ``GraphFolderLoader``, then resize and
    conversion of a chunk of whole mini-batches in two batched launches."""

    def __iter__(self):
        samples = self.dataset.samples
        epoch = self._next_epoch()
        batches = self.index_batches()
        per = max(1, self.chunk // self.batch_size)
        groups = [batches[i:i + per] for i in range(0, len(batches), per)]
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            def decode(group):
                return [pool.submit(load_rgb, samples[i][0]) for b in group for i in b]

            pending = decode(groups[0]) if groups else []
            for c, group in enumerate(groups):
                images = [f.result() for f in pending]
                pending = decode(groups[c + 1]) if c + 1 < len(groups) else []
                tensors = self._build(images, [i for b in group for i in b], epoch)
                del images
                at = 0
                for b in group:
                    yield tensors[at:at + len(b)], torch.tensor([samples[i][1] for i in b], dtype=torch.long)
                    at += len(b)
