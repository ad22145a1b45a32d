"""The dataset's augmentation branch on the device (the part that is off by default in this fork:
config/FusionTransformerConfig.py:88-97).

3-D (data/utils/augmentation_3d.py:4-53, called from semantic_kitti_dataloader.py:216-217): noisy rotation, axis flips, rotation
about z, random translation inside the receptive field.  The RANDOM DRAWS stay on the host -- `draw_augmentation_3d` consumes
`numpy.random` in exactly the order the reference does, so a seeded run picks the same matrix and offset --; what is applied to the
points runs on the GPU with numpy's float32 / float64 rounding (`augment_and_scale_3d`): bit-exact against the reference function run in
the build container (tests/golden/voxel_coords_augmented.npz).

2-D (semantic_kitti_dataloader.py:166-212): bottom crop with the point filter, left-right flip with the column update, normalisation,
HWC -> CHW (`augment_image`); `draw_augmentation_2d` makes the two draws.  That dataloader class cannot be imported here (torchvision,
torchsparse), so the 2-D part is checked against a numpy restatement of its statements: PARITY UNPINNED, though every operation is an
index or a float32 subtraction and division.

Colour jitter (:117,146,196-197, `T.ColorJitter(*color_jitter)` on the cropped PIL image; config key
DATASET.SemanticKITTISCN.augmentation.color_jitter, off by default): `augment_image_u8(..., jitter=draw_color_jitter(*cfg))` runs it on
the device (`ftx_color_jitter_chw`), fused with the float conversion, flip, normalisation and HWC -> CHW.  What is pinned: the image
operations, bit-exact against the installed Pillow's uint8 arithmetic (ImageEnhance.Brightness / Contrast / Color and the HSV round
trip of adjust_hue) on all 2^24 colours and on full frames (tests/test_color_jitter_gpu.py, tests/golden/color_jitter.npz).  What is not:
the draws, which restate torchvision 0.8.2 (not importable here) -- [upstream, not in container] PARITY OF THE DRAW ORDER UNPINNED --
and the reference era's Pillow and torch RNG versions, which are not installed either.

Resize (data/nuscenes/nuscenes_dataloader.py:175-185, `image.resize(self.resize, Image.BILINEAR)` on every 1600 x 900 camera frame and the
two statements that rescale the projected points, before jitter, / 255, flip and normalisation): `augment_image_u8(..., resize=(w, h))`,
or `functional.resize_bilinear_u8` and `resize_points_img` on their own.  What is pinned: the image bytes, bit-exact against the installed
Pillow 12.2.0's 8-bit bilinear resample (integer arithmetic on a coefficient table built in double: include/ftx.h) on full frames, both
directions, every row alignment of a crop view (tests/test_resize_host.py, tests/test_resize_gpu.py, tests/golden/resize_bilinear.npz);
the points against numpy's rounding of the two statements.  What is not: the reference era's Pillow is not installed, so its 8bpc
resample could not be run here -- PARITY WITH THAT VERSION UNPINNED."""
from __future__ import annotations

import numpy as np
import torch

from .. import functional as spf

__all__ = ["draw_augmentation_3d", "augment_and_scale_3d", "draw_augmentation_2d", "augment_image", "draw_color_jitter",
           "resize_points_img", "augment_image_u8"]


def draw_augmentation_3d(noisy_rot=0.0, flip_x=0.0, flip_y=0.0, rot_z=0.0, transl=False, rng=np.random):
    """The random numbers of one call of the reference's augment_and_scale_3d, drawn in its order (augmentation_3d.py:22-51):
    randn(3, 3) for the noisy rotation, one randint(0, 2) per enabled flip, rand() for the z angle, rand(3) for the translation.
    Returns (rot (3,3) float32 or None, transl_u (3,) float64 or None).  `rng`: numpy.random or a RandomState."""
    rot = None
    if noisy_rot > 0 or flip_x > 0 or flip_y > 0 or rot_z > 0:
        rot = np.eye(3, dtype=np.float32)
        if noisy_rot > 0:
            rot += rng.randn(3, 3) * noisy_rot                 # float64 noise added into the float32 matrix
        if flip_x > 0:
            rot[0][0] *= rng.randint(0, 2) * 2 - 1
        if flip_y > 0:
            rot[1][1] *= rng.randint(0, 2) * 2 - 1
        if rot_z > 0:
            theta = rng.rand() * rot_z
            zr = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]], dtype=np.float32)
            rot = rot.dot(zr)
    u = rng.rand(3) if transl else None
    return rot, u


def augment_and_scale_3d(points: torch.Tensor, scale, full_scale, rot=None, transl_u=None) -> torch.Tensor:
    """points (N,3) float32 on the GPU -> float voxel coordinates, as the reference's function with the draws made by
    draw_augmentation_3d: points . rot (libftx, the sgemm's fused rounding), * scale, translation to the positive octant, and the
    random offset `clip(full_scale - max - 0.001, 0) * u` added in float64 and rounded back to float32 (numpy's in-place add of a
    float64 array into a float32 one)."""
    if not points.is_cuda or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("augment_and_scale_3d: expected a (N,3) float32 CUDA tensor")
    if rot is not None:
        points = spf.rotate_points(points.contiguous(), rot)
    coords = points * float(scale)
    coords = coords - coords.min(0).values
    if transl_u is not None:
        room = torch.clamp((float(full_scale) - coords.max(0).values) - 0.001, min=0.0)          # float32 throughout, like numpy's weak scalars
        offset = room.double() * torch.as_tensor(np.asarray(transl_u, dtype=np.float64), device=points.device)
        coords = (coords.double() + offset).float()
    return coords


def draw_augmentation_2d(image_size, bottom_crop=None, fliplr=None, rng=np.random):
    """The draws of semantic_kitti_dataloader.py:170-197 in order: the crop's left edge (if bottom_crop = (width, height)), then the
    flip decision (if fliplr is a probability).  image_size = (width, height) of the uncropped image.  Returns (crop box
    (left, top, right, bottom) or None, flip: bool)."""
    box = None
    if bottom_crop is not None:
        left = int(rng.rand() * (image_size[0] + 1 - bottom_crop[0]))
        box = (left, image_size[1] - bottom_crop[1], left + bottom_crop[0], image_size[1])
    flip = (fliplr is not None) and bool(rng.rand() < fliplr)
    return box, flip


def augment_image(image: torch.Tensor, points_img: torch.Tensor, box=None, flip=False, normalizer=None):
    """image (H,W,3) float32 in [0,1] on the GPU, points_img (N,2) float (row, col).  Returns (img (3,h,w) float32, img_indices (K,2)
    int64, keep (N,) bool): crop + point filter + shift (:176-190), truncation to int64 (:193), flip with `w - 1 - col` (:201-203),
    (image - mean) / std (:206-210), HWC -> CHW (:212).  `keep` is what the caller applies to points / feats / labels (:187-190)."""
    keep = torch.ones((points_img.shape[0],), dtype=torch.bool, device=points_img.device)
    pi = points_img
    if box is not None:
        left, top, right, bottom = box
        keep = (pi[:, 0] >= top) & (pi[:, 0] < bottom) & (pi[:, 1] >= left) & (pi[:, 1] < right)
        image = image[top:bottom, left:right]
        pi = pi[keep].clone()
        pi[:, 0] -= top
        pi[:, 1] -= left
    idx = pi.to(torch.int64)
    if flip:
        image = torch.flip(image, dims=(1,))
        idx = idx.clone()
        idx[:, 1] = image.shape[1] - 1 - idx[:, 1]
    if normalizer is not None:
        mean, std = normalizer
        mean = torch.as_tensor(np.asarray(mean, dtype=np.float32), device=image.device)
        std = torch.as_tensor(np.asarray(std, dtype=np.float32), device=image.device)
        image = (image - mean) / std
    return image.permute(2, 0, 1).contiguous(), idx, keep


def _jitter_range(value, name, center=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True):
    """torchvision 0.8.2 ColorJitter._check_input."""
    import numbers
    if isinstance(value, numbers.Number):
        if value < 0:
            raise ValueError("If {} is a single number, it must be non negative.".format(name))
        value = [center - float(value), center + float(value)]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        if not bound[0] <= value[0] <= value[1] <= bound[1]:
            raise ValueError("{} values should be between {}".format(name, bound))
    else:
        raise TypeError("{} should be a single number or a list/tuple with length 2.".format(name))
    if value[0] == value[1] == center:  # brightness / contrast / saturation (1, 1) or hue (0, 0): the op is off
        value = None
    return value


def draw_color_jitter(brightness=0, contrast=0, saturation=0, hue=0, generator=None):
    """The draws of one `T.ColorJitter(brightness, contrast, saturation, hue)(img)` call (semantic_kitti_dataloader.py:146,197), as
    torchvision 0.8.2 makes them: `torch.randperm(4)` picks the order, then each op that is not off draws its factor with
    `torch.tensor(1.0).uniform_(lo, hi).item()` when its turn comes.  Returns the ordered list of (op, factor), op one of
    "brightness", "contrast", "saturation", "hue" -- what `augment_image_u8(jitter=...)` and functional.color_jitter_* take.
    Torch's CPU generator (`generator`, or the global one) is the only source: numpy.random is not touched, so the crop and flip draws
    of draw_augmentation_2d see the same stream with jitter on or off.
    [upstream, not in container] PARITY OF THE DRAW ORDER UNPINNED: torchvision is not importable here; this restates its code."""
    ranges = [_jitter_range(brightness, "brightness"), _jitter_range(contrast, "contrast"), _jitter_range(saturation, "saturation"),
              _jitter_range(hue, "hue", center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)]
    names = ("brightness", "contrast", "saturation", "hue")
    out = []
    for fn_id in torch.randperm(4, generator=generator).tolist():
        r = ranges[fn_id]
        if r is None:
            continue
        f = torch.tensor(1.0).uniform_(r[0], r[1], generator=generator).item()
        if fn_id == 3 and not -0.5 <= f <= 0.5:  # F.adjust_hue's check, raised when the op is applied
            raise ValueError("hue_factor ({}) is not in [-0.5, 0.5].".format(f))
        out.append((names[fn_id], f))
    return out


def resize_points_img(points_img: torch.Tensor, image_size, resize) -> torch.Tensor:
    """The two statements of nuscenes_dataloader.py:181-182 with numpy's rounding: points_img (N, 2) float (row, col) of a frame of
    image_size = (width, height) that is resized to resize = (width, height); row' = float(resize[1]) / image_size[1] * floor(row), the
    same with index 0 for the columns.  The Python scalar is a weak scalar to numpy: for float32 points the product is
    float32(scalar) * floor(p) rounded once in float32 (not the float64 product rounded to float32: they differ on non-dyadic ratios), for
    float64 points it is the float64 product.  Returns the scaled points as a new tensor on the points' device; the truncation to int64
    stays with the caller."""
    if not isinstance(points_img, torch.Tensor) or points_img.dtype not in (torch.float32, torch.float64) or points_img.dim() != 2 \
            or points_img.shape[1] != 2:
        raise ValueError("resize_points_img: expected a (N, 2) float32 or float64 tensor")
    sy = float(resize[1]) / image_size[1]
    sx = float(resize[0]) / image_size[0]
    if points_img.dtype == torch.float32:
        sy, sx = float(np.float32(sy)), float(np.float32(sx))  # exact in float32: one rounding, that of the product
    fl = torch.floor(points_img)
    return torch.stack([fl[:, 0] * sy, fl[:, 1] * sx], 1)


def augment_image_u8(image_u8: torch.Tensor, points_img: torch.Tensor, box=None, flip=False, normalizer=None, jitter=None, resize=None):
    """augment_image for the uint8 frame the dataloader holds as a PIL image, with the optional colour jitter in its place: crop
    (a view, no copy), jitter (:197, after the crop), np.array(image, float32) / 255 (:199), flip, normalisation, HWC -> CHW -- the image
    part in one device call (functional.color_jitter_to_chw), the points exactly as augment_image.  `jitter`: the list of
    draw_color_jitter, or None.  With jitter=None the image equals augment_image(u8 / 255) with the division correctly rounded
    (numpy's; note that torch's GPU `u8.float() / 255` multiplies by a rounded reciprocal instead and differs in the last bit).
    `resize` = (width, height), the NuScenes loader's first step (nuscenes_dataloader.py:175-185): if the frame's size differs, the
    points are rescaled (resize_points_img) and the frame is resized (functional.resize_bilinear_u8, bit-exact with PIL's
    Image.BILINEAR) before everything else; enlarging raises ValueError (the loader asserts image.size[0] > resize[0]).  A `box` then
    counts in the resized frame's coordinates (no reference loader combines the two).  resize=None changes nothing."""
    if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8 or image_u8.dim() != 3:
        raise ValueError("augment_image_u8: expected an (H, W, 3) uint8 tensor")
    if resize is not None:
        size = (image_u8.shape[1], image_u8.shape[0])
        resize = (int(resize[0]), int(resize[1]))
        if size != resize:
            if not size[0] > resize[0]:
                raise ValueError(f"augment_image_u8: resize {resize} would enlarge a frame of {size}")
            points_img = resize_points_img(points_img, size, resize)
            image_u8 = spf.resize_bilinear_u8(image_u8, resize)
    keep = torch.ones((points_img.shape[0],), dtype=torch.bool, device=points_img.device)
    pi = points_img
    image = image_u8
    if box is not None:
        left, top, right, bottom = box
        keep = (pi[:, 0] >= top) & (pi[:, 0] < bottom) & (pi[:, 1] >= left) & (pi[:, 1] < right)
        image = image[top:bottom, left:right]
        pi = pi[keep].clone()
        pi[:, 0] -= top
        pi[:, 1] -= left
    idx = pi.to(torch.int64)
    if flip:
        idx = idx.clone()
        idx[:, 1] = image.shape[1] - 1 - idx[:, 1]
    img = spf.color_jitter_to_chw(image, jitter, flip, normalizer)
    return img, idx, keep
