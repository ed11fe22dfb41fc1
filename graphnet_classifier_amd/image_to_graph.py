"""Device-side image -> graph builders (drop-in counterparts of the reference's ``utils/image_to_graph``).

Same function names and arguments as the reference
(``image_to_graph_optimized.py:7,42,50``, ``image_to_graph_patch.py:6``, ``image_to_graph_superpixel.py:8``);
the single-image builders decode and resize on the host with PIL exactly as the reference does, then everything else
(SLIC segmentation, node features, positions, edges) is produced in HBM by the kernels of ``csrc/superpixel.hip``
and ``csrc/graph_build.hip``.  Results
are the tensors ``utils/dataloader.py:49-51`` would build: ``x`` float32, ``pos`` float32, ``edge_index``
int64, already on the GPU, in the reference's node and edge order.

``resize`` is Pillow's ``Image.resize`` on the device (csrc/resize.hip) for a batch of decoded images of any sizes, and
``graphs_from_images`` builds the graphs of such a batch from it: the same tensors as the single-image builders, with
the resize and SLIC run as batched launches.  ``crop_resize`` and ``color_jitter`` (csrc/augment.hip, K25) are Pillow's
``crop().resize()`` / ``FLIP_LEFT_RIGHT`` and ``ImageEnhance`` chains on the device, byte for byte; with the parameters an
``augment.Augmentation`` samples they take the place of the resize (``augmentation=`` of the batch builders).
"""
from __future__ import annotations

import collections
import functools

import numpy as np
import torch

from . import functional as F
from . import native
from .MLP import default_device


def _device() -> torch.device:
    dev = default_device()
    if dev.type != "cuda":
        raise RuntimeError("image_to_graph: no GPU visible and no CPU fallback exists")
    return dev


def _load_resized(image_or_path, resize_value: int) -> np.ndarray:
    """optimized.py:65-70 / patch.py:18-24 / superpixel.py:21-26: PIL RGB, resize, uint8 [H, W, 3]."""
    from PIL import Image
    image = Image.open(image_or_path).convert("RGB") if isinstance(image_or_path, str) else image_or_path.convert("RGB")
    return np.array(image.resize((resize_value, resize_value)))


def create_grid_edges_optimized(H: int, W: int, diagonals: bool = False) -> torch.Tensor:
    """int64 [2, E] on the GPU; same edge order as optimized.py:7-39."""
    lib = native.load_library()
    dev = _device()
    e = lib.gnc_grid_num_edges(H, W, int(bool(diagonals)))
    ei = torch.empty(2, e, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        native._check(lib.gnc_grid_edges_i64(H, W, int(bool(diagonals)), ei.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream), "gnc_grid_edges_i64")
    return ei


@functools.lru_cache(maxsize=128)
def get_cached_edge_index(resize_value: int, diagonals: bool) -> torch.Tensor:
    """optimized.py:42-47: one topology per image size."""
    return create_grid_edges_optimized(resize_value, resize_value, diagonals)


def _to_device_u8(img: np.ndarray) -> torch.Tensor:
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError("expected a uint8 [H, W, C] image")
    return torch.from_numpy(np.ascontiguousarray(img)).to(_device())


def pixel_graph_from_array(img_u8: np.ndarray, diagonals: bool = False, use_cache: bool = True):
    return _pixel_graph(_to_device_u8(img_u8), diagonals, use_cache)


def _pixel_graph(img: torch.Tensor, diagonals: bool, use_cache: bool, with_edges: bool = True):
    """pixel graph of a device uint8 [H, W, C] image (``with_edges=False``: the nodes alone, ``edge_index`` is None)"""
    lib = native.load_library()
    H, W, C = img.shape
    x = torch.empty(H * W, C, dtype=torch.float32, device=img.device)
    pos = torch.empty(H * W, 2, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        native._check(lib.gnc_pixel_nodes_f32(img.data_ptr(), H, W, C, x.data_ptr(), pos.data_ptr(),
                                              torch.cuda.current_stream(img.device).cuda_stream), "gnc_pixel_nodes_f32")
    if not with_edges:
        return x, pos, None
    ei = get_cached_edge_index(H, bool(diagonals)) if (use_cache and H == W) else create_grid_edges_optimized(H, W, diagonals)
    return x, pos, ei


def image_to_graph_pixel_optimized(image_or_path, resize_value: int = 128, diagonals: bool = False, use_cache: bool = True):
    """optimized.py:50-87."""
    return pixel_graph_from_array(_load_resized(image_or_path, resize_value), diagonals, use_cache)


def patch_graph_from_array(img_u8: np.ndarray, patch_size: int = 8):
    return _patch_graph(_to_device_u8(img_u8), patch_size)


def _patch_graph(img: torch.Tensor, patch_size: int, with_edges: bool = True):
    """patch graph of a device uint8 [H, W, C] image (``with_edges=False``: the nodes alone, ``edge_index`` is None)"""
    lib = native.load_library()
    H, W, C = img.shape
    nh, nw = H // patch_size, W // patch_size
    x = torch.empty(nh * nw, C, dtype=torch.float32, device=img.device)
    pos = torch.empty(nh * nw, 2, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        native._check(lib.gnc_patch_nodes_f32(img.data_ptr(), H, W, C, patch_size, x.data_ptr(), pos.data_ptr(),
                                              torch.cuda.current_stream(img.device).cuda_stream), "gnc_patch_nodes_f32")
    return x, pos, (create_grid_edges_optimized(nh, nw, False) if with_edges else None)


def image_to_graph_patch(image_or_path, resize_value: int = 128, patch_size: int = 8):
    """patch.py:6-54."""
    return patch_graph_from_array(_load_resized(image_or_path, resize_value), patch_size)


NODE_FEATURES = (None, "descriptor")
# the columns of a region descriptor (csrc/region_descriptor.hip, DESIGN K26), GNC_REGION_DESCRIPTOR_DIM of them
DESCRIPTOR_COLUMNS = ("mean_r", "mean_g", "mean_b", "std_r", "std_g", "std_b", "area", "bbox_height", "bbox_width",
                      "spread_y", "spread_x", "box_fill", "boundary", "texture_r", "texture_g", "texture_b")
REGION_DESCRIPTOR_DIM = len(DESCRIPTOR_COLUMNS)
# what one launch of gnc_region_descriptors_rgb_u8 takes: the limits of the batched region-graph build
REGION_DESCRIPTOR_MAX_PIXELS, REGION_DESCRIPTOR_MAX_NODES = 65536, 512


def check_node_features(node_features, method: str = "superpixel") -> None:
    """The ``node_features`` keyword of the superpixel builders, ``graphs_from_images`` and ``GraphImageFolder``."""
    if node_features not in NODE_FEATURES:
        raise ValueError(f"Unknown node_features: {node_features!r} (None: the method's own node features; 'descriptor': "
                         f"the {REGION_DESCRIPTOR_DIM} region descriptor columns of a superpixel graph)")
    if node_features is not None and method != "superpixel":
        raise ValueError(f"node_features={node_features!r} needs method='superpixel', got method={method!r}: a pixel has no "
                         "extent, and patch descriptors are not implemented")


def _region_descriptors_launch(img: torch.Tensor, labels: torch.Tensor, node_capacity: int):
    """ONE launch over a contiguous device batch ``[B, H, W, 3]`` uint8 / ``[B, H, W]`` int32: ``(desc [B, cap, 16], counts [B, 3])``."""
    lib = native.load_library()
    B, H, W, _ = img.shape
    with torch.cuda.device(img.device):
        nbytes = lib.gnc_region_descriptors_workspace_bytes(B, H, W, node_capacity)
        if nbytes == 0:
            raise NotImplementedError(f"region_descriptors: {B} images of {H} x {W} at {node_capacity} nodes is outside the "
                                      f"supported set (H*W <= {REGION_DESCRIPTOR_MAX_PIXELS}, {REGION_DESCRIPTOR_MAX_NODES} nodes)")
        desc = torch.empty(B, node_capacity, REGION_DESCRIPTOR_DIM, dtype=torch.float32, device=img.device)
        counts = torch.empty(B, 3, dtype=torch.int32, device=img.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        native._check(lib.gnc_region_descriptors_rgb_u8(labels.data_ptr(), img.data_ptr(), B, H, W, node_capacity,
                                                        desc.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,
                                                        torch.cuda.current_stream(img.device).cuda_stream),
                      "gnc_region_descriptors_rgb_u8")
    return desc, counts


def region_descriptors(images_u8, labels, node_capacity: int | None = None):
    """Region descriptors of label images (csrc/region_descriptor.hip, K26): for every region of ``labels`` the 16 float32 columns
    ``DESCRIPTOR_COLUMNS`` - mean colour (the plain superpixel ``x``, bit for bit), colour standard deviation, area share,
    bounding-box extent, spatial spread, box fill, boundary share and texture - all in [0, 1], from exact integer sums.

    ``images_u8`` ``[B, H, W, 3]`` uint8 with ``labels`` ``[B, H, W]`` (values in ``[0, H W)``, gaps allowed; row ``i`` is node ``i``
    of the region graph of the same labels): ``desc [B, node_capacity, 16]`` and int32 ``counts [B, 3]`` = (regions, bad-label flag,
    overflow flag) on the device, ONE launch and no host synchronisation; rows behind an image's region count are zeros, and an
    image with a flag set holds zeros only.  ``node_capacity`` defaults to 512, the most one launch takes.

    One image ``[H, W, 3]`` with ``[H, W]`` labels: ``desc [regions, 16]`` (this form reads the count; a label outside
    ``[0, H W)`` raises ``ValueError``, more regions than the capacity ``NotImplementedError``) and ``counts [3]``."""
    img = images_u8 if isinstance(images_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images_u8))
    if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise ValueError("region_descriptors: expected a uint8 RGB image [H, W, 3] or batch [B, H, W, 3]")
    single = img.dim() == 3
    img = (img.unsqueeze(0) if single else img).to(_device()).contiguous()
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
    lab = lab.unsqueeze(0) if single and lab.dim() == 2 else lab
    if tuple(lab.shape) != tuple(img.shape[:3]):
        raise ValueError("region_descriptors: expected label images of the images' size")
    lab = lab.to(device=img.device, dtype=torch.int32).contiguous()
    cap = REGION_DESCRIPTOR_MAX_NODES if node_capacity is None else int(node_capacity)
    desc, counts = _region_descriptors_launch(img, lab, cap)
    if not single:
        return desc, counts
    regions, bad, overflow = (int(v) for v in counts[0].tolist())
    if bad:
        raise ValueError("label image has values outside [0, H*W)")
    if overflow:
        raise NotImplementedError(f"region_descriptors: {regions} regions do not fit node_capacity = {cap} (at most "
                                  f"{REGION_DESCRIPTOR_MAX_NODES} regions and H*W <= {REGION_DESCRIPTOR_MAX_PIXELS})")
    return desc[0, :regions], counts[0]


def superpixel_graph_from_labels(img_u8: np.ndarray, segments: np.ndarray, node_features=None):
    """Everything of superpixel.py after the SLIC call (:33-71) for a given label image: per-segment mean
    colour (of img/255) and centroid, region adjacency, edges [i,j],[j,i] in lexicographic order.
    ``node_features="descriptor"``: ``x`` is the region descriptor ``[nodes, 16]`` (``region_descriptors``), whose first three
    columns are the plain ``x``."""
    check_node_features(node_features)
    img = _to_device_u8(img_u8)
    H, W, C = img.shape
    if C != 3 or segments.shape != (H, W):
        raise ValueError("expected an RGB image and a label image of the same size")
    labels = torch.from_numpy(np.ascontiguousarray(segments.astype(np.int32))).to(img.device)
    return _superpixel_graph_from_device_labels(img, labels, node_features)


def _superpixel_graph_from_device_labels(img_u8, labels: torch.Tensor, node_features=None):
    lib = native.load_library()
    img = img_u8 if isinstance(img_u8, torch.Tensor) else _to_device_u8(img_u8)
    H, W, C = img.shape
    labels = labels.to(device=img.device, dtype=torch.int32).contiguous()
    n = H * W
    desc = None
    if node_features is not None:  # one more launch off the same labels, in front of the one host read
        if n > REGION_DESCRIPTOR_MAX_PIXELS:
            raise NotImplementedError(_descriptor_limits(f"an image of {H} x {W}"))
        desc, _ = _region_descriptors_launch(img.contiguous().unsqueeze(0), labels.unsqueeze(0), REGION_DESCRIPTOR_MAX_NODES)
    x = torch.empty(n, 3, dtype=torch.float32, device=img.device)
    pos = torch.empty(n, 2, dtype=torch.float32, device=img.device)
    ei = torch.empty(2, 4 * n, dtype=torch.int64, device=img.device)
    counts = torch.empty(3, dtype=torch.int32, device=img.device)
    with torch.cuda.device(img.device):
        nbytes = lib.gnc_rag_workspace_bytes(H, W)
        if nbytes == 0:
            native._check(-1, "gnc_rag_workspace_bytes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        native._check(lib.gnc_rag_build(labels.data_ptr(), img.data_ptr(), H, W, x.data_ptr(), pos.data_ptr(), ei.data_ptr(),
                                        4 * n, counts.data_ptr(), ws.data_ptr(), nbytes,
                                        torch.cuda.current_stream(img.device).cuda_stream), "gnc_rag_build")
    s, e, bad = (int(v) for v in counts.tolist())  # one host sync: the sizes are data dependent
    if bad:
        raise ValueError("label image has values outside [0, H*W)")
    if desc is not None:
        if s > REGION_DESCRIPTOR_MAX_NODES:
            raise NotImplementedError(_descriptor_limits(f"a graph of {s} regions"))
        return desc[0, :s], pos[:s], ei[:, :e]
    return x[:s], pos[:s], ei[:, :e]


def _descriptor_limits(what: str) -> str:
    return (f"node_features='descriptor': {what} is outside what the descriptor kernel takes (at most "
            f"{REGION_DESCRIPTOR_MAX_NODES} regions and H*W <= {REGION_DESCRIPTOR_MAX_PIXELS})")


def slic(image_u8, n_segments: int = 100, compactness: float = 10, max_iter: int = 10,
         enforce_connectivity: bool = True, min_size_factor: float = 0.5, max_size_factor: float = 3,
         start_label: int = 0, return_counts: bool = False):
    """scikit-image 0.18.3 ``slic(img_as_float(img), ...)`` on the GPU (csrc/superpixel.hip) for uint8 RGB images
    ``[H, W, 3]`` or a batch ``[B, H, W, 3]`` (NumPy array or tensor).  Returns int32 labels ``[H, W]`` / ``[B, H, W]``
    on the device, and with ``return_counts`` also the int32 ``[B]`` number of labels per image.  sigma = 0, no mask,
    unit spacing, Lab conversion, SLIC (not SLIC-zero): the options the reference uses (superpixel.py:31)."""
    lib = native.load_library()
    img = image_u8 if isinstance(image_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image_u8))
    if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise ValueError("slic: expected a uint8 RGB image [H, W, 3] or batch [B, H, W, 3]")
    single = img.dim() == 3
    img = (img.unsqueeze(0) if single else img).to(_device()).contiguous()
    B, H, W, _ = img.shape
    if B == 0 or H == 0 or W == 0:
        raise ValueError("slic: empty image or batch")
    labels = torch.empty(B, H, W, dtype=torch.int32, device=img.device)
    counts = torch.empty(B, dtype=torch.int32, device=img.device)
    with torch.cuda.device(img.device):
        nbytes = lib.gnc_slic_workspace_bytes(B, H, W, int(n_segments))
        if nbytes == 0:
            raise NotImplementedError(f"slic: {H} x {W} with n_segments={n_segments} is outside the supported set")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        native._check(lib.gnc_slic_rgb_u8(img.data_ptr(), B, H, W, int(n_segments), float(compactness), int(max_iter),
                                          int(bool(enforce_connectivity)), float(min_size_factor),
                                          float(max_size_factor), int(start_label), labels.data_ptr(),
                                          counts.data_ptr(), ws.data_ptr(), nbytes,
                                          torch.cuda.current_stream(img.device).cuda_stream), "gnc_slic_rgb_u8")
    if single:
        labels, counts = labels[0], counts[:1]
    return (labels, counts) if return_counts else labels


SuperpixelGraphBatch = collections.namedtuple("SuperpixelGraphBatch", "x pos edge_index counts")

# what one launch of gnc_rag_build_batched takes (csrc/rag_batched.hip)
RAG_BATCHED_MAX_NODES, RAG_BATCHED_MAX_EDGES = 512, 4096


def superpixel_capacities(n_segments: int) -> tuple[int, int]:
    """Node and edge capacities of the batched region-graph build for ``slic(n_segments=...)`` images, chosen on the
    host.  SLIC hands out about ``n_segments`` labels (its grid rounds, and the connectivity pass merges and splits: the
    fixture graphs have 0.69 - 1.19 x n_segments nodes), a planar region adjacency has fewer than 3 undirected = 6
    directed edges per node (the fixtures: 4.5 - 4.9).  1.5 x and 8 x leave room on both; a graph that still does not fit
    is flagged by the kernel and built by the per-image path."""
    n = max(1, int(n_segments))
    nodes = min(RAG_BATCHED_MAX_NODES, (n * 3 // 2 + 31) // 32 * 32)
    edges = min(RAG_BATCHED_MAX_EDGES, (nodes * 8 + 255) // 256 * 256)
    return nodes, edges


def superpixel_graphs_batched(images_u8, labels=None, *, n_segments: int = 100, compactness: float = 10,
                              node_capacity: int, edge_capacity: int, node_features=None) -> SuperpixelGraphBatch:
    """Region graphs of a batch of resized uint8 RGB images ``[B, H, W, 3]`` in ONE launch (csrc/rag_batched.hip), with
    no host synchronisation: ``x [B, node_capacity, 3]``, ``pos [B, node_capacity, 2]``, ``edge_index [B, 2,
    edge_capacity]`` and int32 ``counts [B, 4]`` = (nodes, directed edges, bad-label flag, overflow flag) on the device.
    ``labels`` ``[B, H, W]`` given: the segmentation to use; otherwise the batched ``slic(n_segments, compactness)``.

    Image ``b``'s graph is ``x[b, :nodes]``, ``pos[b, :nodes]``, ``edge_index[b, :, :edges]`` and equals
    ``superpixel_graph_from_labels`` of that image bit for bit; rows behind it are 0, edge slots -1.  An image whose
    overflow flag is set reports its true sizes (edges = -1 above 512 nodes) and holds padding only.

    ``node_features="descriptor"`` (K26): ``x`` is ``[B, node_capacity, 16]``, the region descriptors of the same labels
    (``region_descriptors``: one more launch, still no host synchronisation), so ``x[..., :3]`` is the plain ``x``; ``pos``,
    ``edge_index`` and ``counts`` are those of the plain build.  The descriptor kernel knows no edge capacity: an image that
    overflows on its edges alone keeps its descriptor rows, one with more nodes than ``node_capacity`` holds zeros."""
    check_node_features(node_features)
    lib = native.load_library()
    img = images_u8 if isinstance(images_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images_u8))
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] != 3:
        raise ValueError("superpixel_graphs_batched: expected a uint8 RGB batch [B, H, W, 3]")
    img = img.to(_device()).contiguous()
    B, H, W, _ = img.shape
    if labels is None:
        labels = slic(img, n_segments=n_segments, compactness=compactness, start_label=0)
    elif not isinstance(labels, torch.Tensor):
        labels = torch.from_numpy(np.ascontiguousarray(labels))
    if tuple(labels.shape) != (B, H, W):
        raise ValueError("superpixel_graphs_batched: expected label images [B, H, W] of the images' size")
    labels = labels.to(device=img.device, dtype=torch.int32).contiguous()
    node_capacity, edge_capacity = int(node_capacity), int(edge_capacity)
    with torch.cuda.device(img.device):
        nbytes = lib.gnc_rag_batched_workspace_bytes(B, H, W, node_capacity, edge_capacity)
        if nbytes == 0:
            raise NotImplementedError(f"superpixel_graphs_batched: {B} images of {H} x {W} at {node_capacity} nodes / "
                                      f"{edge_capacity} edges is outside the supported set (H*W <= 65536, "
                                      f"{RAG_BATCHED_MAX_NODES} nodes, {RAG_BATCHED_MAX_EDGES} edges)")
        x = torch.empty(B, node_capacity, 3, dtype=torch.float32, device=img.device)
        pos = torch.empty(B, node_capacity, 2, dtype=torch.float32, device=img.device)
        ei = torch.empty(B, 2, edge_capacity, dtype=torch.int64, device=img.device)
        counts = torch.empty(B, 4, dtype=torch.int32, device=img.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        native._check(lib.gnc_rag_build_batched(labels.data_ptr(), img.data_ptr(), B, H, W, node_capacity, edge_capacity,
                                                x.data_ptr(), pos.data_ptr(), ei.data_ptr(), counts.data_ptr(),
                                                ws.data_ptr(), nbytes, torch.cuda.current_stream(img.device).cuda_stream),
                      "gnc_rag_build_batched")
    if node_features is not None:
        x, _ = _region_descriptors_launch(img, labels, node_capacity)
    return SuperpixelGraphBatch(x, pos, ei, counts)


def _superpixel_graphs_from_device_batch(imgs: torch.Tensor, labels: torch.Tensor, node_capacity: int, edge_capacity: int, knn=None,
                                         node_features=None):
    """The loader's list of ``(x, pos, edge_index)`` for a device batch: one batched build, ONE host read of the sizes;
    an image that does not fit the capacities (or a batch outside the kernel's supported set) takes the per-image path.
    ``knn = (k, pos_weight)``: the edges are the k nearest neighbours instead (K24), one more launch over the padded batch, off
    its device node counts and in front of the same single host read.  ``node_features="descriptor"`` (K26): one more launch
    off the same labels and capacities, in front of that read too; the kNN space stays (colour, position) = ``x[..., :3]``."""
    B, H, W, _ = imgs.shape

    def per_image(im, lab):
        x, pos, ei = _superpixel_graph_from_device_labels(im, lab, node_features)
        return (x, pos, ei) if knn is None else (x, pos, _knn_edges_of_graph(x[:, :3], pos, "superpixel", H, *knn))

    if native.load_library().gnc_rag_batched_workspace_bytes(B, H, W, node_capacity, edge_capacity) == 0:
        return [per_image(im, lab) for im, lab in zip(imgs, labels)]
    batch = superpixel_graphs_batched(imgs, labels, node_capacity=node_capacity, edge_capacity=edge_capacity,
                                      node_features=node_features)
    if knn is not None:
        k = knn[0]
        knn_ei, _, _ = native.knn_graph_padded(knn_features(batch.x[..., :3], batch.pos, "superpixel", H, knn[1]), batch.counts, k)
    graphs = []
    for b, (s, e, bad, overflow) in enumerate(batch.counts.tolist()):  # the chunk's one host sync
        if bad:
            raise ValueError("label image has values outside [0, H*W)")
        if overflow:
            graphs.append(per_image(imgs[b], labels[b]))
        elif knn is not None:
            _check_knn_nodes(s, k)
            graphs.append((batch.x[b, :s].contiguous(), batch.pos[b, :s].contiguous(), knn_ei[b, :, :k * s].contiguous()))
        else:  # contiguous copies: the topology cache and the capture's copies see what the per-image path hands them
            graphs.append((batch.x[b, :s].contiguous(), batch.pos[b, :s].contiguous(), batch.edge_index[b, :, :e].contiguous()))
    return graphs


def superpixel_graph_from_array(img_u8: np.ndarray, n_segments: int = 100, compactness: float = 10, node_features=None):
    """superpixel.py:29-71 for an already resized uint8 RGB array: device SLIC, then the region graph
    (``node_features="descriptor"``: with the region descriptors as ``x``, K26)."""
    check_node_features(node_features)
    labels = slic(img_u8, n_segments=n_segments, compactness=compactness, start_label=0)
    return _superpixel_graph_from_device_labels(img_u8, labels, node_features)


def image_to_graph_superpixel(image_or_path, resize_value: int = 128, n_segments: int = 100, compactness: int = 10,
                              node_features=None, **slic_options):
    """superpixel.py:8-73, SLIC included, on the device.  Options of scikit-image's ``slic`` that the reference never
    passes (mask, sigma, spacing, slic_zero, ...) are not implemented and raise.  ``node_features="descriptor"`` (K26): ``x`` is
    the ``[nodes, 16]`` region descriptor instead of the mean colour, which stays its first three columns."""
    check_node_features(node_features)
    if slic_options:
        raise NotImplementedError(f"image_to_graph_superpixel: SLIC options {sorted(slic_options)} are not implemented "
                                  "(the reference passes only n_segments and compactness)")
    return superpixel_graph_from_array(_load_resized(image_or_path, resize_value), n_segments, compactness, node_features)


# PIL.Image.Resampling values; the device resize implements the three whose weights need no sin / cos
_RESAMPLE = {"bilinear": 2, "bicubic": 3, "box": 4}
_UNSUPPORTED_RESAMPLE = {"nearest": 0, "lanczos": 1, "antialias": 1, "hamming": 5}


def _resample_code(resample) -> int:
    if isinstance(resample, str):
        name = resample.lower()
        if name in _RESAMPLE:
            return _RESAMPLE[name]
        if name in _UNSUPPORTED_RESAMPLE:
            raise NotImplementedError(f"resize: resample={resample!r} is not implemented (bicubic, bilinear, box)")
        raise ValueError(f"resize: unknown resample {resample!r}")
    code = int(resample)
    if code in _RESAMPLE.values():
        return code
    if code in _UNSUPPORTED_RESAMPLE.values():
        raise NotImplementedError(f"resize: resample={resample!r} is not implemented (bicubic, bilinear, box)")
    raise ValueError(f"resize: unknown resample {resample!r}")


def _as_u8_tensor(img, who: str = "resize") -> torch.Tensor:
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dtype != torch.uint8:
        raise TypeError(f"{who}: expected uint8 images, got {t.dtype}")
    return t


def _upload(t: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """host -> device through pinned memory, stream-ordered (no host wait); device tensors pass through"""
    if t.is_cuda:
        return t.to(dev)
    return t.contiguous().pin_memory().to(dev, non_blocking=True)


def _gather_images(images, dev: torch.device, who: str):
    """The images of ``resize`` / ``crop_resize`` on the device: ``(src, rows, single)``.  ``rows`` is None for a dense
    ``[B, H, W, 3]`` ``src``; for a list of images of different sizes ``src`` is their bytes back to back and ``rows`` the host
    list of ``[byte offset, h, w]`` per image (the kernels' size table)."""
    if isinstance(images, (list, tuple)):
        if not images:
            raise ValueError(f"{who}: empty list of images")
        imgs = [_as_u8_tensor(im, who) for im in images]
        for im in imgs:
            if im.dim() != 3 or im.shape[-1] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError(f"{who}: expected RGB images [H, W, 3], got {tuple(im.shape)}")
        if all(im.shape == imgs[0].shape for im in imgs):
            src = torch.stack([_upload(im, dev) for im in imgs]) if imgs[0].is_cuda else _upload(torch.stack(imgs), dev)
            return src, None, False
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
        offs = np.cumsum([0] + [h * w * 3 for h, w in sizes])
        if all(im.is_cuda for im in imgs):
            src = torch.cat([im.to(dev).reshape(-1) for im in imgs])
        else:
            src = _upload(torch.cat([im.cpu().reshape(-1) for im in imgs]), dev)
        return src, [[int(o), h, w] for o, (h, w) in zip(offs[:-1], sizes)], False
    t = _as_u8_tensor(images, who)
    if t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError(f"{who}: expected an RGB image [H, W, 3] or batch [B, H, W, 3], got {tuple(t.shape)}")
    single = t.dim() == 3
    src = _upload(t.unsqueeze(0) if single else t, dev).contiguous()
    if src.shape[0] == 0 or src.shape[1] == 0 or src.shape[2] == 0:
        raise ValueError(f"{who}: empty image or batch")
    return src, None, single


def _batch_extent(src: torch.Tensor, rows):
    """``(B, in_h, in_w)`` of a gathered batch: the largest image sides of a mixed-size one"""
    if rows is None:
        return int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    return len(rows), max(r[1] for r in rows), max(r[2] for r in rows)


def resize(images, size, resample="bicubic", box=None, reducing_gap=None) -> torch.Tensor:
    """``PIL.Image.fromarray(img).resize(size, resample)`` on the GPU, byte for byte, for a batch of RGB images.

    ``images``: one uint8 ``[H, W, 3]`` array or tensor, a ``[B, H, W, 3]`` batch, or a list of ``[H_i, W_i, 3]``
    images of different sizes (NumPy arrays or tensors, on the host or the device).  ``size`` is ``(W, H)`` as in
    PIL.  Returns a device uint8 ``[B, H, W, 3]`` tensor, or ``[H, W, 3]`` for a single image.  Host images are
    uploaded through pinned memory; the whole batch is one stream-ordered enqueue with no host synchronisation, and a
    dense device batch can be resized under ``torch.cuda.graph`` capture.

    ``resample``: ``"bicubic"`` (Pillow's default), ``"bilinear"`` or ``"box"``, or the matching
    ``PIL.Image.Resampling`` values.  ``NEAREST``, ``HAMMING`` and ``LANCZOS`` raise ``NotImplementedError``
    (Hamming and Lanczos weights need ``sin`` / ``cos``, and the device libm is not promised to match glibc's last
    bit), as do the ``box`` and ``reducing_gap`` arguments of ``Image.resize``."""
    if box is not None or reducing_gap is not None:
        raise NotImplementedError("resize: the box and reducing_gap arguments of Image.resize are not implemented")
    code = _resample_code(resample)
    out_w, out_h = (int(v) for v in size)
    if out_w < 1 or out_h < 1:
        raise ValueError(f"resize: output size must be positive, got {tuple(size)}")
    dev = _device()
    lib = native.load_library()
    src, rows, single = _gather_images(images, dev, "resize")
    table = None if rows is None else _upload(torch.tensor(rows, dtype=torch.int64), dev)
    B, in_h, in_w = _batch_extent(src, rows)
    out = torch.empty(B, out_h, out_w, 3, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nbytes = lib.gnc_resize_workspace_bytes(B, in_h, in_w, out_h, out_w, code)
        if nbytes == 0:
            raise NotImplementedError(f"resize: {B} images of up to {in_h} x {in_w} -> {out_h} x {out_w} is outside "
                                      "the supported set (batch and sides up to 65535)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        native._check(lib.gnc_resize_rgb_u8(src.data_ptr(), table.data_ptr() if table is not None else None, B, in_h,
                                            in_w, out_h, out_w, code, out.data_ptr(), ws.data_ptr(), nbytes,
                                            torch.cuda.current_stream(dev).cuda_stream), "gnc_resize_rgb_u8")
    return out[0] if single else out


def crop_resize(images, boxes, size, resample="bicubic", flip=None) -> torch.Tensor:
    """``Image.fromarray(img_b).crop(box_b).resize(size, resample)`` and, where ``flip[b]`` is set,
    ``.transpose(Image.Transpose.FLIP_LEFT_RIGHT)``, on the GPU, byte for byte (csrc/augment.hip, K25).

    ``images`` and ``size`` as in ``resize``.  ``boxes``: a host integer array ``[B, 4]`` of ``(left, top, right, bottom)`` per image
    (``[4]`` for a single image), ``flip``: a host bool array ``[B]`` or None.  An empty box, a box that leaves its image or a length
    that does not match the batch raises ``ValueError``.  This is *crop, then resize*: filter windows are clamped at the box, where
    ``Image.resize(box=...)`` reads the pixels around it.  Boxes and flags travel with the size table in one pinned upload; the
    launches are those of ``resize`` (the flip is part of the last store), stream-ordered without a host synchronisation.  For a
    replay under ``torch.cuda.graph`` pass ``boxes`` (int64 ``[B, 4]``) and ``flip`` as DEVICE tensors beside a dense device batch:
    they are then not checked on the host, and a row the kernel finds outside its image leaves its output as it was."""
    code = _resample_code(resample)
    out_w, out_h = (int(v) for v in size)
    if out_w < 1 or out_h < 1:
        raise ValueError(f"crop_resize: output size must be positive, got {tuple(size)}")
    dev = _device()
    lib = native.load_library()
    src, rows, single = _gather_images(images, dev, "crop_resize")
    B, in_h, in_w = _batch_extent(src, rows)
    if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
        if boxes.dtype != torch.int64 or tuple(boxes.shape) != (B, 4):
            raise ValueError(f"crop_resize: device boxes must be int64 [{B}, 4], got {boxes.dtype} {tuple(boxes.shape)}")
        if flip is None:
            flip = torch.zeros(B, dtype=torch.int64, device=dev)
        if not (isinstance(flip, torch.Tensor) and flip.is_cuda and tuple(flip.shape) == (B,)):
            raise ValueError(f"crop_resize: with device boxes, flip must be a device tensor [{B}]")
        table = None if rows is None else _upload(torch.tensor(rows, dtype=torch.int64), dev)
        box_table = torch.cat([boxes.to(dev), flip.to(dev, torch.int64).view(B, 1)], dim=1).contiguous()
    else:
        bx = np.asarray(boxes)
        if bx.dtype.kind not in "iu":
            raise ValueError(f"crop_resize: boxes must be integers, got {bx.dtype}")
        bx = bx.astype(np.int64).reshape(1, -1) if single and bx.ndim == 1 else bx.astype(np.int64)
        if bx.shape != (B, 4):
            raise ValueError(f"crop_resize: {B} images need boxes [{B}, 4], got {tuple(bx.shape)}")
        fl = np.zeros(B, np.int64) if flip is None else np.asarray(flip).astype(bool).astype(np.int64).reshape(-1)
        if fl.shape != (B,):
            raise ValueError(f"crop_resize: {B} images need {B} flip flags, got {tuple(fl.shape)}")
        hw = np.array([[r[1], r[2]] for r in rows], np.int64) if rows is not None else np.array([[in_h, in_w]] * B, np.int64)
        bad = ~((bx[:, 0] >= 0) & (bx[:, 1] >= 0) & (bx[:, 0] < bx[:, 2]) & (bx[:, 1] < bx[:, 3]) & (bx[:, 2] <= hw[:, 1])
                & (bx[:, 3] <= hw[:, 0]))
        if bad.any():
            b = int(np.flatnonzero(bad)[0])
            raise ValueError(f"crop_resize: box {tuple(int(v) for v in bx[b])} of image {b} is empty or leaves its "
                             f"{int(hw[b, 0])} x {int(hw[b, 1])} image")
        # one upload: the size table (mixed sizes only), then the (left, top, right, bottom, flip) rows
        host = np.concatenate([np.asarray(rows if rows is not None else [], np.int64).reshape(-1),
                               np.concatenate([bx, fl[:, None]], axis=1).reshape(-1)])
        both = _upload(torch.from_numpy(host), dev)
        table = None if rows is None else both[:3 * B]
        box_table = both[both.numel() - 5 * B:]
    out = torch.empty(B, out_h, out_w, 3, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nbytes = lib.gnc_crop_resize_workspace_bytes(B, in_h, in_w, out_h, out_w, code)
        if nbytes == 0:
            raise NotImplementedError(f"crop_resize: {B} images of up to {in_h} x {in_w} -> {out_h} x {out_w} is outside "
                                      "the supported set (batch and sides up to 65535)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        native._check(lib.gnc_crop_resize_rgb_u8(src.data_ptr(), table.data_ptr() if table is not None else None,
                                                 box_table.data_ptr(), B, in_h, in_w, out_h, out_w, code, out.data_ptr(),
                                                 ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream),
                      "gnc_crop_resize_rgb_u8")
    return out[0] if single else out


JITTER_OPS = ("brightness", "contrast", "saturation")  # the operation codes 0, 1, 2 of ``order``


def _jitter_factors(value, B: int, name: str) -> np.ndarray:
    f = np.asarray(value, dtype=np.float32)
    if f.ndim == 0:
        f = np.full(B, f, np.float32)
    if f.shape != (B,):
        raise ValueError(f"color_jitter: {name} must be a scalar or [{B}], got {tuple(f.shape)}")
    if not np.all(np.isfinite(f)) or (f < 0).any():
        raise ValueError(f"color_jitter: {name} factors must be finite and >= 0")
    return f


def color_jitter(batch_u8, brightness=None, contrast=None, saturation=None, order=None) -> torch.Tensor:
    """Pillow's ``ImageEnhance.Brightness`` / ``.Contrast`` / ``.Color`` on the GPU, byte for byte, for a dense uint8 batch
    ``[B, H, W, 3]`` (or one ``[H, W, 3]`` image): every image gets its own float32 factors (``[B]`` or a scalar; None leaves the
    operation out) in its own order.  ``order``: host ``[B, 3]`` (or ``[3]``), per image a permutation of ``(0, 1, 2)`` =
    ``(brightness, contrast, saturation)``, first to last; the default is that order.  Returns a new tensor: one copy and ONE
    launch in place on it (csrc/augment.hip), no host synchronisation.  Contrast's grey level is the rounded mean L of the image
    as the operations in front of it left it, as in a chain of ``enhance`` calls.  With no operation the copy is returned as it is."""
    t = _as_u8_tensor(batch_u8, "color_jitter")
    if t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError(f"color_jitter: expected an RGB image [H, W, 3] or batch [B, H, W, 3], got {tuple(t.shape)}")
    single = t.dim() == 3
    dev = _device()
    if t.is_cuda:
        out = (t.unsqueeze(0) if single else t).to(dev).contiguous().clone()
    else:
        out = _upload(t.unsqueeze(0) if single else t, dev)
    B, H, W = int(out.shape[0]), int(out.shape[1]), int(out.shape[2])
    if B == 0 or H == 0 or W == 0:
        raise ValueError("color_jitter: empty image or batch")
    given = (brightness, contrast, saturation)
    factors = np.ones((B, 3), np.float32)
    for op, (value, name) in enumerate(zip(given, JITTER_OPS)):
        if value is not None:
            factors[:, op] = _jitter_factors(value, B, name)
    if order is None:
        perm = np.tile(np.arange(3, dtype=np.int32), (B, 1))
    else:
        perm = np.asarray(order)
        if perm.dtype.kind not in "iu":
            raise ValueError(f"color_jitter: order must be integers, got {perm.dtype}")
        perm = np.tile(perm.astype(np.int32), (B, 1)) if perm.ndim == 1 else perm.astype(np.int32)
        if perm.shape != (B, 3) or (np.sort(perm, axis=1) != np.arange(3)).any():
            raise ValueError(f"color_jitter: order must hold a permutation of (0, 1, 2) per image, [{B}, 3]")
    perm = np.where(np.array([v is not None for v in given])[perm], perm, -1).astype(np.int32)  # left-out operations
    if (perm < 0).all():
        return out[0] if single else out
    lib = native.load_library()
    host = np.concatenate([perm.reshape(-1), factors.reshape(-1).view(np.int32)])  # one upload: order, then the factors' bits
    both = _upload(torch.from_numpy(host), dev)
    with torch.cuda.device(dev):
        native._check(lib.gnc_color_jitter_rgb_u8(out.data_ptr(), B, H, W, both.data_ptr(), both[3 * B:].data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "gnc_color_jitter_rgb_u8")
    return out[0] if single else out


def _augmented(images_u8, resize_value: int, resample: str, augmentation) -> torch.Tensor:
    """The chunk's ``resize`` with sampled augmentation parameters (``augment.AugmentParams``): ``crop_resize`` and, if any factor
    was drawn, ``color_jitter``."""
    if len(augmentation.boxes) != len(images_u8):
        raise ValueError(f"augmentation holds parameters of {len(augmentation.boxes)} images, the batch has {len(images_u8)}")
    imgs = crop_resize(list(images_u8), augmentation.boxes, (resize_value, resize_value), resample, augmentation.flips)
    if augmentation.brightness is None and augmentation.contrast is None and augmentation.saturation is None:
        return imgs
    return color_jitter(imgs, augmentation.brightness, augmentation.contrast, augmentation.saturation, augmentation.order)


def collate_graphs(graphs):
    """A list of ``(x, pos, edge_index)`` graphs as ONE block-diagonal ``synthetic.GraphBatch``: ``x`` and ``pos`` concatenated,
    node ids of graph g shifted by the nodes in front of it, ``graph_ptr`` / ``edge_ptr`` int64 [G + 1] (host tensors, from the
    shapes).  One concatenation per tensor and one add on the tensors' own device: no per-graph launches, no host
    synchronisation.  ``batch.slice_graphs(g, g + 1)`` gives graph g back; ``CombinedModel.forward_batched(batch.x, batch.pos,
    batch.edge_index, graph_ptr=batch.graph_ptr)`` runs the batch."""
    from .synthetic import GraphBatch
    graphs = list(graphs)
    if not graphs:
        raise ValueError("collate_graphs: empty list of graphs")
    nodes = torch.tensor([0] + [int(g[0].size(0)) for g in graphs], dtype=torch.int64)
    edges = torch.tensor([0] + [int(g[2].size(1)) for g in graphs], dtype=torch.int64)
    graph_ptr, edge_ptr = nodes.cumsum(0), edges.cumsum(0)
    x = torch.cat([g[0] for g in graphs])
    pos = torch.cat([g[1] for g in graphs])
    edge_index = torch.cat([g[2] for g in graphs], dim=1)
    shift = torch.repeat_interleave(graph_ptr[:-1], edges[1:])  # [E] on the host: sizes only, no tensor is read back
    if edge_index.is_cuda:
        shift = shift.pin_memory().to(edge_index.device, non_blocking=True)
    return GraphBatch(x, pos, edge_index + shift, graph_ptr, edge_ptr)


def tensors_from_images(images_u8, resize_value: int = 128, *, augmentation=None) -> torch.Tensor:
    """torchvision's ``Compose([Resize((R, R)), ToTensor()])`` (main.py:13-16 of the reference) for a batch of decoded uint8 RGB
    images ``[H_i, W_i, 3]`` of any sizes: float32 ``[B, 3, R, R]`` on the device, values in [0, 1].  ``Resize`` on a PIL image is
    Pillow's BILINEAR ``Image.resize`` (``resize`` here, byte for byte), ``ToTensor`` is ``permute(2, 0, 1).float().div(255)``
    (``native.u8_hwc_to_f32_chw``, bit for bit): two batched enqueues, no host synchronisation.

    ``augmentation`` (K25): the parameters ``augment.Augmentation.sample`` drew for these images; the resize then is ``crop_resize``
    (BILINEAR) followed by ``color_jitter``, as Pillow would produce them, and ``ToTensor`` is unchanged."""
    if len(images_u8) == 0:
        raise ValueError("tensors_from_images: empty list of images")
    if augmentation is not None:
        return native.u8_hwc_to_f32_chw(_augmented(images_u8, resize_value, "bilinear", augmentation))
    return native.u8_hwc_to_f32_chw(resize(list(images_u8), (resize_value, resize_value), "bilinear"))


METHODS = ("pixel", "patch", "superpixel")


def graphs_from_images(images_u8, method: str = "pixel", resize_value: int = 128, diagonals: bool = False,
                       use_cache: bool = True, n_segments: int = 100, patch_size: int = 8, compactness: float = 10, *,
                       node_capacity: int | None = None, edge_capacity: int | None = None, edges=None, knn_k: int = 8,
                       knn_pos_weight: float = 1.0, augmentation=None, node_features=None):
    """Graphs of a batch of decoded uint8 RGB images ``[H_i, W_i, 3]`` (any sizes): a list of ``(x, pos, edge_index)``
    equal to ``image_to_graph_pixel_optimized`` / ``image_to_graph_patch`` / ``image_to_graph_superpixel`` of each
    image, with arguments named as ``utils/dataloader.py``'s ``OptimizedDatasetLoader``.  The resize of the whole
    batch is one launch (``resize``), superpixel runs one batched ``slic`` and one batched region-graph build
    (``superpixel_graphs_batched`` at capacities derived from ``n_segments``) with ONE host synchronisation per call for
    the graphs' sizes, which depend on the data; pixel and patch nodes are one launch per image.  A superpixel image
    that does not fit the capacities is built by the per-image path (one more synchronisation each);
    ``node_capacity`` / ``edge_capacity`` override the derived capacities (the result does not depend on them).

    ``edges="knn"`` (K24) keeps every method's nodes (``x``, ``pos`` bit for bit) and replaces its edge list by the ``knn_k``
    nearest neighbours of each node in ``knn_features`` (colour next to ``knn_pos_weight`` x position): ``knn_k n`` edges,
    receiver-major.  One more launch per chunk and no further host synchronisation: superpixel chunks run the padded kNN entry
    off the batch's device counts in front of the one host read, pixel and patch chunks one call over the collated nodes.  A
    graph with ``n <= knn_k`` nodes raises ``ValueError``.  ``edges=None`` is the method's own edge list.

    ``augmentation`` (K25): the parameters ``augment.Augmentation.sample`` drew for these images.  The one ``resize`` call then is
    ``crop_resize`` (random resized crop and horizontal flip) followed by ``color_jitter``: the graphs are those of the images
    Pillow produces with the same parameters, and everything behind the resize is unchanged.  None: no new launch.

    ``node_features="descriptor"`` (K26, ``method="superpixel"`` only; another method raises ``ValueError``): ``x`` is the
    ``[nodes, 16]`` region descriptor (``region_descriptors``; ``x[:, :3]`` is the plain ``x``), ``pos`` and ``edge_index`` are
    unchanged - ``edges="knn"`` still looks for neighbours in (colour, position).  One more launch per chunk in front of the same
    single host read; an image on the per-image path runs the kernel alone, and one with more than 512 regions or
    ``H W > 65536`` raises ``NotImplementedError``."""
    if method not in METHODS:
        raise ValueError(f"Unknown method: {method}")
    check_edges(edges, knn_k)
    check_node_features(node_features, method)
    if len(images_u8) == 0:
        return []
    if augmentation is not None:
        imgs = _augmented(images_u8, resize_value, "bicubic", augmentation)
    else:
        imgs = resize(list(images_u8), (resize_value, resize_value))
    if method in ("pixel", "patch"):
        grid = edges is None  # under "knn" the grid's edge list is not built at all
        graphs = [_pixel_graph(im, diagonals, use_cache, grid) if method == "pixel" else _patch_graph(im, patch_size, grid) for im in imgs]
        if grid:
            return graphs
        # one kNN launch over the chunk's collated nodes (same-sized images: the sizes are host values), then split per image
        n = graphs[0][0].size(0)
        _check_knn_nodes(n, knn_k)
        feat = knn_features(torch.cat([g[0] for g in graphs]), torch.cat([g[1] for g in graphs]), method, resize_value, knn_pos_weight)
        ei = F.knn_graph(feat, knn_k, graph_ptr=torch.arange(len(graphs) + 1, dtype=torch.int64) * n)
        ei = (ei.view(2, len(graphs), knn_k * n) - (torch.arange(len(graphs), device=ei.device) * n).view(1, -1, 1))
        return [(x, pos, ei[:, b].contiguous()) for b, (x, pos, _) in enumerate(graphs)]
    labels = slic(imgs, n_segments=n_segments, compactness=compactness, start_label=0)
    nodes, cap_edges = superpixel_capacities(n_segments)
    return _superpixel_graphs_from_device_batch(imgs, labels, nodes if node_capacity is None else int(node_capacity),
                                                cap_edges if edge_capacity is None else int(edge_capacity),
                                                knn=None if edges is None else (knn_k, knn_pos_weight),
                                                node_features=node_features)


EDGES = (None, "knn")


def check_edges(edges, knn_k) -> None:
    """The ``edges`` / ``knn_k`` keywords of ``graphs_from_images`` and ``GraphImageFolder``."""
    if edges not in EDGES:
        raise ValueError(f"Unknown edges: {edges!r} (None: the method's own edges; 'knn': k nearest neighbours)")
    if edges == "knn" and (isinstance(knn_k, bool) or not isinstance(knn_k, int) or not 1 <= knn_k <= native.KNN_MAX_K):
        raise ValueError(f"knn_k must be an integer in [1, {native.KNN_MAX_K}], got {knn_k!r}")


def _check_knn_nodes(n: int, k: int) -> None:
    if n <= k:
        raise ValueError(f"a graph of {n} nodes has fewer than knn_k = {k} other nodes to choose neighbours from; lower knn_k")


def knn_features(x: torch.Tensor, pos: torch.Tensor, method: str, resize_value: int, pos_weight: float = 1.0) -> torch.Tensor:
    """The joint (colour, position) space in which ``edges="knn"`` looks for neighbours: ``[..., 5]`` float32 = the node colours
    scaled to [0, 1] (pixel and patch ``x`` is 0 .. 255 and is divided by 255; superpixel ``x`` already is a mean of ``img / 255``)
    next to ``pos / resize_value * pos_weight``.  ``pos_weight`` is the one knob: 0 gives pure colour neighbours, a large value
    pure spatial ones.  Element-wise, so a batch ``[B, n, .]`` gives each image the bits it gets alone."""
    if method not in METHODS:
        raise ValueError(f"Unknown method: {method}")
    colour = x if method == "superpixel" else x / 255.0
    return torch.cat([colour, pos / float(resize_value) * float(pos_weight)], dim=-1)


def _knn_edges_of_graph(x, pos, method, resize_value, k, pos_weight):
    _check_knn_nodes(x.size(0), k)
    return F.knn_graph(knn_features(x, pos, method, resize_value, pos_weight), k)


def knn_edges(x: torch.Tensor, pos: torch.Tensor, k: int = 8, method: str = "superpixel", resize_value: int = 128,
              pos_weight: float = 1.0) -> torch.Tensor:
    """``edge_index`` int64 [2, k n] of ONE image graph's nodes: every node receives from its ``k`` nearest nodes in
    ``knn_features`` (``functional.knn_graph``: receiver-major, ties by the smaller node id, no self-loops)."""
    check_edges("knn", k)
    return _knn_edges_of_graph(x, pos, method, resize_value, k, pos_weight)
