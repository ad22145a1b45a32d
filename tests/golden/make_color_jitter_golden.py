"""Writes tests/golden/color_jitter.npz: Pillow's colour jitter (the statements of torchvision 0.8.2's ColorJitter on a PIL image:
ImageEnhance.Brightness / Contrast / Color and adjust_hue's HSV round trip) on small seeded uint8 frames, for a set of draw lists.

Uses Pillow, numpy and torch's CPU generator only.  `python tests/golden/make_color_jitter_golden.py` from the repository root."""
import itertools
import os
import sys

import numpy as np
import torch
import PIL
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fusiontransformer_amd.data.augment import draw_color_jitter  # noqa: E402

OPS = ("brightness", "contrast", "saturation", "hue")


def pil_jitter(img, draws):
    """torchvision 0.8.2 functional_pil.adjust_* applied in order."""
    for op, f in draws:
        if op == "brightness":
            img = ImageEnhance.Brightness(img).enhance(f)
        elif op == "contrast":
            img = ImageEnhance.Contrast(img).enhance(f)
        elif op == "saturation":
            img = ImageEnhance.Color(img).enhance(f)
        else:
            h, s, v = img.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            np_h += np.uint8(int(f * 255) % 256)   # np.uint8(negative float) wrapped in reference-era numpy; numpy 2 raises
            img = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return img


def draw_lists():
    g = torch.Generator().manual_seed(20261016)
    lists = [draw_color_jitter(0.4, 0.4, 0.4, generator=g) for _ in range(6)]
    lists += [draw_color_jitter(0.4, 0.4, 0.4, 0.1, generator=g) for _ in range(6)]
    # every order of the four ops, factors from ranges whose ends are exactly 0 and above 1
    for k, perm in enumerate(itertools.permutations(range(4))):
        f = torch.empty(4).uniform_(0.0, 2.2, generator=g).tolist()
        fac = {0: f[0], 1: f[1], 2: f[2], 3: (f[3] / 2.2 - 0.5)}
        if k % 6 == 0:
            fac[perm[0]] = 0.0 if perm[0] != 3 else -0.5
        if k % 6 == 1:
            fac[perm[-1]] = 1.37 if perm[-1] != 3 else 0.5
        lists.append([(OPS[i], float(fac[i])) for i in perm])
    return lists


def main():
    rng = np.random.default_rng(7)
    frame = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    frame[:6] //= 3                                   # a dark band: the contrast mean is not ~127
    wide = rng.integers(0, 256, (30, 61, 3), dtype=np.uint8)
    crop = (5, 9, 38, 30)                             # (left, top, right, bottom): odd offset, width 33
    lists = draw_lists()
    ops = np.full((len(lists), 4), -1, dtype=np.int32)
    factors = np.zeros((len(lists), 4), dtype=np.float64)
    out_frame, out_crop = [], []
    view = np.ascontiguousarray(wide[crop[1]:crop[3], crop[0]:crop[2]])
    for i, dl in enumerate(lists):
        for j, (op, f) in enumerate(dl):
            ops[i, j], factors[i, j] = OPS.index(op), f
        out_frame.append(np.asarray(pil_jitter(Image.fromarray(frame), dl)))
        out_crop.append(np.asarray(pil_jitter(Image.fromarray(view), dl)))
    path = os.path.join(ROOT, "tests", "golden", "color_jitter.npz")
    np.savez_compressed(path, frame=frame, wide=wide, crop=np.asarray(crop, dtype=np.int64), ops=ops, factors=factors,
                        out_frame=np.stack(out_frame), out_crop=np.stack(out_crop), pillow_version=np.asarray(PIL.__version__))
    print(path, len(lists), "draw lists", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
