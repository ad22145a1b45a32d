"""Colour jitter on the device (csrc/ftx_image.hip) against Pillow: the committed golden outputs, every colour per op, full frames,
the whole augment_image_u8 against the dataloader's statements, and no host synchronisation."""
import os

import numpy as np
import pytest
import torch

from fusiontransformer_amd import functional as spf
from fusiontransformer_amd.data.augment import augment_image, augment_image_u8, draw_augmentation_2d, draw_color_jitter

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_jitter.npz")
NAMES = ("brightness", "contrast", "saturation", "hue")


def _pil():
    return pytest.importorskip("PIL.Image"), pytest.importorskip("PIL.ImageEnhance")


def pil_jitter(img_u8, draws):
    """torchvision 0.8.2 functional_pil.adjust_* in order, on a PIL image made from a uint8 HWC array."""
    Image, ImageEnhance = _pil()
    img = Image.fromarray(np.ascontiguousarray(img_u8))
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
            np_h += np.uint8(int(f * 255) % 256)
            img = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return np.asarray(img)


def all_colours():
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_golden_fixture():
    """Every frame and draw list of tests/golden/color_jitter.npz (made with Pillow) bit for bit, through both entry points."""
    g = np.load(GOLDEN)
    frame = torch.from_numpy(g["frame"]).cuda()
    wide = torch.from_numpy(g["wide"]).cuda()
    left, top, right, bottom = (int(v) for v in g["crop"])
    view = wide[top:bottom, left:right]
    assert view.stride(0) != 3 * view.shape[1] and not view.is_contiguous()
    assert len(g["ops"]) >= 30
    for i in range(len(g["ops"])):
        draws = [(NAMES[o], float(f)) for o, f in zip(g["ops"][i], g["factors"][i]) if o >= 0]
        for src, want in ((frame, g["out_frame"][i]), (view, g["out_crop"][i])):
            got = spf.color_jitter_u8(src, draws).cpu().numpy()
            assert np.array_equal(got, want), (i, draws, int((got != want).sum()))
            chw = spf.color_jitter_to_chw(src, draws).cpu().numpy()
            assert np.array_equal(chw, np.moveaxis(want.astype(np.float32) / np.float32(255), -1, 0)), i


def test_every_colour_per_op_against_pillow():
    img = all_colours()
    dev = torch.from_numpy(img).cuda()
    for op in ("brightness", "saturation"):
        for f in (0.0, 0.6, 0.999, 1.0, 1.37, 1.4):
            got = spf.color_jitter_u8(dev, [(op, f)]).cpu().numpy()
            want = pil_jitter(img, [(op, f)])
            assert np.array_equal(got, want), (op, f, int((got != want).any(-1).sum()))
    # |hue_factor| <= 0.5 reaches int(f * 255) in -127..127, so every shift but 128 (f = 0.5 gives 127, f = -0.5 gives 129)
    for shift in (0, 1, 127, 129, 255):
        f = (shift + 0.5) / 255 if shift < 128 else (shift - 256 - 0.5) / 255
        assert int(f * 255) % 256 == shift
        got = spf.color_jitter_u8(dev, [("hue", f)]).cpu().numpy()
        want = pil_jitter(img, [("hue", f)])
        assert np.array_equal(got, want), (shift, int((got != want).any(-1).sum()))


def test_contrast_mean_on_the_rounding_edge():
    """Images whose mean luma is exactly k + 0.5 and one pixel's worth either side of it: int(mean + 0.5) decides the grey level."""
    rng = np.random.default_rng(1)
    h, w = 64, 100
    n = h * w
    for k in (0, 63, 127, 200):
        for delta in (-1, 0, 1):
            target = (2 * k + 1) * n // 2 + delta                   # luma sum: mean = k + 0.5 + delta / n
            l = np.full(n, target // n, dtype=np.int64)
            l[: target - l.sum()] += 1
            assert l.sum() == target and l.max() <= 255
            perm = rng.permutation(n)
            grey = l[perm].astype(np.uint8).reshape(h, w)
            img = np.repeat(grey[..., None], 3, -1)                  # grey pixels: convert("L") returns the value itself
            for f in (0.0, 0.5, 1.37):
                got = spf.color_jitter_u8(torch.from_numpy(img).cuda(), [("contrast", f)]).cpu().numpy()
                want = pil_jitter(img, [("contrast", f)])
                assert np.array_equal(got, want), (k, delta, f)


@pytest.mark.parametrize("shape", ["full", "crop"])
def test_full_chains_on_realistic_frames(shape):
    rng = np.random.default_rng(2 if shape == "full" else 3)
    H, W = 370, 1226
    base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    base[:120] = (base[:120].astype(np.int32) * 3 // 4 + 40).astype(np.uint8)  # not uniform noise: a brighter band on top
    dev = torch.from_numpy(base).cuda()
    g = torch.Generator().manual_seed(17)
    np.random.seed(4)
    for i in range(50):
        if shape == "full":
            src, ref = dev, base
        else:
            box, _ = draw_augmentation_2d((W, H), (480, 302), None)
            left, top, right, bottom = box
            src, ref = dev[top:bottom, left:right], base[top:bottom, left:right]
            assert src.stride(0) == 3 * W
        draws = draw_color_jitter(0.4, 0.4, 0.4, 0.1 if i % 2 else 0, generator=g)
        got = spf.color_jitter_u8(src, draws).cpu().numpy()
        want = pil_jitter(ref, draws)
        assert np.array_equal(got, want), (i, draws, int((got != want).any(-1).sum()))


def test_augment_image_u8_matches_the_dataloader_statements():
    """crop, jitter (:197), np.array(image, float32) / 255 (:199), flip, normalise, HWC -> CHW -- restated in numpy with Pillow for the
    jitter -- and, without jitter, augment_image on u8 / 255 bit for bit."""
    rng = np.random.default_rng(5)
    H, W, n = 370, 1226, 5000
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    points_img = np.stack([rng.uniform(0, H, n), rng.uniform(0, W, n)], 1).astype(np.float32)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    dev_img, dev_pts = torch.from_numpy(image).cuda(), torch.from_numpy(points_img).cuda()
    g = torch.Generator().manual_seed(9)
    for seed, crop, fliplr, jit in ((1, (480, 302), 0.5, True), (2, (480, 302), 1.0, True), (3, None, 1.0, True), (4, None, None, False),
                                    (5, (480, 302), 1.0, False)):
        np.random.seed(seed)
        box, flip = draw_augmentation_2d((W, H), crop, fliplr)
        jitter = draw_color_jitter(0.4, 0.4, 0.4, 0.1, generator=g) if jit else None
        np.random.seed(seed)
        img, pi, keep = image, points_img.copy(), np.ones(n, dtype=bool)
        if crop is not None:
            left = int(np.random.rand() * (W + 1 - crop[0])); right = left + crop[0]; top = H - crop[1]; bottom = H
            keep = (pi[:, 0] >= top) & (pi[:, 0] < bottom) & (pi[:, 1] >= left) & (pi[:, 1] < right)
            img = img[top:bottom, left:right]
            pi = pi[keep]
            pi[:, 0] -= top
            pi[:, 1] -= left
        if jitter:
            img = pil_jitter(img, jitter)
        img = np.array(img, dtype=np.float32) / 255.
        idx = pi.astype(np.int64)
        if (fliplr is not None) and (np.random.rand() < fliplr):
            img = np.ascontiguousarray(np.fliplr(img))
            idx[:, 1] = img.shape[1] - 1 - idx[:, 1]
        img = (img - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
        want = np.moveaxis(img, -1, 0)
        got_img, got_idx, got_keep = augment_image_u8(dev_img, dev_pts, box, flip, (mean, std), jitter)
        assert np.array_equal(got_keep.cpu().numpy(), keep) and np.array_equal(got_idx.cpu().numpy(), idx), seed
        assert got_img.shape == want.shape and np.array_equal(got_img.cpu().numpy(), want), seed
        if not jit:
            f01 = torch.from_numpy(image.astype(np.float32) / np.float32(255)).cuda()
            ref_img, ref_idx, ref_keep = augment_image(f01, dev_pts, box, flip, (mean, std))
            assert torch.equal(ref_img, got_img) and torch.equal(ref_idx, got_idx) and torch.equal(ref_keep, got_keep), seed
            nonorm, _, _ = augment_image_u8(dev_img, dev_pts, box, flip)
            assert torch.equal(nonorm, augment_image(f01, dev_pts, box, flip)[0]), seed


def test_jitter_and_convert_do_not_synchronise():
    rng = np.random.default_rng(6)
    dev = torch.from_numpy(rng.integers(0, 256, (370, 1226, 3), dtype=np.uint8)).cuda()
    view = dev[68:370, 101:581]
    draws = [("saturation", 0.7), ("contrast", 1.3), ("hue", -0.05), ("brightness", 1.1)]
    spf.color_jitter_to_chw(view, draws, True, ([0.5] * 3, [0.25] * 3))           # first call: workspace allocation outside the check
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for d in (draws, draws[1:], [draws[0]], []):
            spf.color_jitter_to_chw(view, d, True, ([0.5] * 3, [0.25] * 3))
            spf.color_jitter_u8(view, d)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
