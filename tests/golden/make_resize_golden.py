"""Writes tests/golden/resize_bilinear.npz: Pillow's `Image.resize(size, Image.BILINEAR)` on small seeded uint8 RGB frames -- both
axes shrunk (even and odd sizes), an enlargement, each axis alone, a frame with saturated bands and checkerboards.  Arrays only:
in_<i>, size_<i> = (width, height), out_<i>.  The numpy restatement the tests use (tests/resize_ref.py) is checked against Pillow here too.

Uses Pillow and numpy only.  `python tests/golden/make_resize_golden.py` from the repository root."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import resize_ref as R  # noqa: E402

CASES = [("random", (160, 90), (40, 23)), ("random", (123, 37), (61, 19)), ("random", (40, 23), (97, 51)), ("random", (96, 54), (48, 54)),
         ("random", (96, 54), (96, 27)), ("bands", (128, 72), (32, 18)), ("bands", (67, 45), (66, 44)), ("random", (33, 9), (1, 1))]


def main():
    rng = np.random.default_rng(20261016)
    out = {"pillow_version": np.array(PIL.__version__)}
    for i, (content, (w, h), size) in enumerate(CASES):
        a = R.random_frame(rng, w, h) if content == "random" else R.banded_frame(rng, w, h)
        want = np.asarray(Image.fromarray(a).resize(size, Image.BILINEAR))
        assert np.array_equal(R.resize(a, size), want), (i, (w, h), size)
        out["in_%d" % i], out["size_%d" % i], out["out_%d" % i] = a, np.array(size, dtype=np.int32), want
    path = os.path.join(ROOT, "tests", "golden", "resize_bilinear.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
