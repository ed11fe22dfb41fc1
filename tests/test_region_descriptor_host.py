"""CPU checks of the region descriptor (DESIGN K26): the NumPy reference of the tests on the superpixel fixtures, the two
symbols of csrc/region_descriptor.hip and their supported set, and the ``node_features`` keyword's argument checks."""
import pathlib
import re

import numpy as np
import pytest

from tests import region_descriptor_reference as R
from tests.test_superpixel_golden import CASES

REPO = pathlib.Path(__file__).resolve().parent.parent


def test_reference_on_every_fixture_segmentation():
    with_graph = regions = 0
    for _, img, labels, _, graph in CASES:
        rows = R.descriptor_rows(img, labels)
        regions += len(rows)
        assert rows.dtype == np.float32 and rows.shape[1] == R.DIM == len(R.COLUMNS)
        assert np.isfinite(rows).all() and rows.min() >= 0.0 and rows.max() <= 1.0
        if graph is not None:
            assert np.array_equal(rows[:, :3], graph[0])  # the plain build's x, bit for bit
            with_graph += 1
    assert len(CASES) == 44 and with_graph == 26 and regions == 4563


def test_reference_on_regions_with_known_values():
    img = np.zeros((4, 6, 3), np.uint8)
    img[:, :, 0] = 255
    img[::2, :, 1] = 255  # rows alternate 255 / 0 in G
    lab = np.zeros((4, 6), np.int32)
    lab[0, 0] = 9  # a single-pixel region; region 0 keeps 23 pixels
    desc, counts = R.region_descriptors(img, lab, 4)
    assert counts.tolist() == [2, 0, 0] and not desc[2:].any()
    one = desc[1]
    assert one[:3].tolist() == [1.0, 1.0, 0.0] and not one[3:6].any() and not one[9:11].any() and not one[13:].any()
    assert one[6] == np.float32(1 / 24) and one[7] == np.float32(1 / 4) and one[8] == np.float32(1 / 6) and one[11] == 1.0 and one[12] == 1.0
    rest = desc[0]
    assert rest[0] == 1.0 and rest[3] == 0.0 and rest[7] == 1.0 and rest[8] == 1.0 and rest[11] == np.float32(23 / 24)
    assert rest[12] == np.float32(2 / 23)  # (0, 1) and (1, 0) touch the single pixel
    pairs = (4 * 5 - 1) + (3 * 6 - 1)  # horizontal and vertical pairs without those through (0, 0)
    assert rest[14] == np.float32((255 * 17 / 255.0) / pairs) and rest[13] == 0.0
    assert R.region_descriptors(img, lab, 1)[1].tolist() == [2, 0, 1] and not R.region_descriptors(img, lab, 1)[0].any()
    lab[3, 5] = 24
    assert R.region_descriptors(img, lab, 4)[1].tolist() == [2, 1, 0] and not R.region_descriptors(img, lab, 4)[0].any()


def test_symbols_exported_at_abi_20():
    from graphnet_classifier_amd import image_to_graph as I2G
    from graphnet_classifier_amd import native
    lib = native.load_library()
    header = (REPO / "include" / "gnc_hip.h").read_text()
    assert lib.gnc_abi_version() == native.ABI_VERSION == 20 and re.search(r"#define\s+GNC_ABI_VERSION\s+20\b", header)
    for name in ("gnc_region_descriptors_workspace_bytes", "gnc_region_descriptors_rgb_u8"):
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name) and name in header
    assert re.search(r"#define\s+GNC_REGION_DESCRIPTOR_DIM\s+16\b", header)
    assert I2G.REGION_DESCRIPTOR_DIM == len(I2G.DESCRIPTOR_COLUMNS) == 16 and tuple(I2G.DESCRIPTOR_COLUMNS) == R.COLUMNS


def test_workspace_query_is_the_supported_set():
    from graphnet_classifier_amd import native
    lib = native.load_library()
    q = lib.gnc_region_descriptors_workspace_bytes
    assert q(1, 256, 256, 512) > 0 and q(1 << 20, 1, 65536, 1) > 0 and q(64, 128, 128, 160) > 0
    assert q(1, 1, 65537, 512) == 0 and b"supported set" in lib.gnc_last_error_string()
    assert q(1, 65537, 1, 512) == 0 and q(1, 257, 256, 512) == 0
    assert q(1, 128, 128, 513) == 0
    assert q(0, 128, 128, 512) == 0 and q(1, 0, 128, 512) == 0 and q(1, 128, 0, 512) == 0 and q(1, 128, 128, 0) == 0
    assert q((1 << 20) + 1, 8, 8, 16) == 0
    GNC_ERR_INVALID_ARGUMENT = -1  # decided before any device work
    assert lib.gnc_region_descriptors_rgb_u8(None, None, 1, 128, 128, 513, None, None, None, 0, None) == GNC_ERR_INVALID_ARGUMENT
    assert lib.gnc_region_descriptors_rgb_u8(None, None, 1, 128, 128, 512, None, None, None, 0, None) == GNC_ERR_INVALID_ARGUMENT


def _folder(tmp_path):
    from PIL import Image
    for cls in ("a", "b"):
        (tmp_path / cls).mkdir()
        Image.fromarray(CASES[0][1]).save(tmp_path / cls / "0.png")
    return str(tmp_path)


@pytest.mark.parametrize("kw,match", [({"method": "superpixel", "node_features": "colour"}, "Unknown node_features"),
                                      ({"method": "superpixel", "node_features": True}, "Unknown node_features"),
                                      ({"method": "pixel", "node_features": "descriptor"}, "method='pixel'"),
                                      ({"method": "patch", "node_features": "descriptor"}, "method='patch'")],
                         ids=["unknown", "bool", "pixel", "patch"])
def test_keyword_errors_before_any_device_work(tmp_path, kw, match):
    from graphnet_classifier_amd import image_to_graph as I2G
    from graphnet_classifier_amd.dataset import GraphImageFolder
    with pytest.raises(ValueError, match=match):
        I2G.graphs_from_images([CASES[0][1]], resize_value=32, **kw)
    with pytest.raises(ValueError, match=match):
        GraphImageFolder(_folder(tmp_path), resize_value=32, **kw)


def test_folder_reports_its_feature_width(tmp_path):
    from graphnet_classifier_amd.dataset import GraphImageFolder
    root = _folder(tmp_path)
    assert GraphImageFolder(root, method="superpixel").num_node_features == 3
    assert GraphImageFolder(root, method="pixel").num_node_features == 3
    ds = GraphImageFolder(root, method="superpixel", node_features="descriptor")
    assert ds.num_node_features == 16 and ds.node_features == "descriptor"
