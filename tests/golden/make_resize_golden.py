#!/usr/bin/env python3
"""Write tests/golden/g11_resize.npz: seeded uint8 RGB inputs and the SHA-256 of Pillow's ``Image.resize`` output for
BICUBIC, BILINEAR and BOX, which pins the semantics csrc/resize.hip follows against a Pillow upgrade.

    python tests/golden/make_resize_golden.py      (recorded with Pillow 12.2.0)

Arrays, one set per case ``<tag>``:

    in_<tag>             uint8 [H, W, 3] input
    size_<tag>           int64 [2]: output (W, H), as PIL takes it
    sha_<tag>_<filter>   uint8 bytes of the hex SHA-256 of the uint8 [H', W', 3] output
"""
import hashlib
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = {"bicubic": Image.Resampling.BICUBIC, "bilinear": Image.Resampling.BILINEAR, "box": Image.Resampling.BOX}
# input (H, W) -> output (W, H): 1 x 1, a row, a column, unchanged, 2x up, 2x down, non-integer both ways, non-square,
# a long horizontal window (1000 -> 16)
CASES = [((1, 1), (4, 3)), ((1, 9), (4, 2)), ((11, 1), (3, 5)), ((19, 23), (23, 19)), ((16, 12), (24, 32)),
         ((48, 64), (32, 24)), ((37, 53), (41, 29)), ((30, 20), (61, 40)), ((5, 1000), (16, 7))]


def main():
    rng = np.random.default_rng(20261016)
    out = {"pillow_version": np.frombuffer(PIL.__version__.encode(), np.uint8)}
    for (h, w), (W, H) in CASES:
        tag = f"{h}x{w}_to_{H}x{W}"
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out["in_" + tag] = img
        out["size_" + tag] = np.array([W, H], np.int64)
        for name, f in FILTERS.items():
            digest = hashlib.sha256(np.array(Image.fromarray(img).resize((W, H), f)).tobytes()).hexdigest()
            out[f"sha_{tag}_{name}"] = np.frombuffer(digest.encode(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "g11_resize.npz"), **out)


if __name__ == "__main__":
    main()
