"""Image resize on the device (csrc/ftx_resize.hip) against Pillow's 8-bit bilinear resample: the committed golden outputs, full
frames against the numpy restatement of tests/resize_ref.py (and Pillow where it is importable), crop views at every byte alignment,
augment_image_u8(resize=...) against the NuScenes loader's statements, no host synchronisation, graph replay, batches.  Every
comparison is equality over the whole array."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fusiontransformer_amd import functional as spf
from fusiontransformer_amd.data.augment import augment_image_u8, draw_color_jitter, resize_points_img
from tests import resize_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_bilinear.npz")


def _pil_image():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def dev_resize(a, size):
    return spf.resize_bilinear_u8(torch.from_numpy(a).cuda(), size).cpu().numpy()


def test_golden_fixture():
    """Every frame of tests/golden/resize_bilinear.npz (inputs and Pillow's outputs; Pillow is not needed here) bit for bit."""
    g = np.load(GOLDEN)
    n = sum(1 for k in g.files if k.startswith("in_"))
    assert n >= 8
    one_axis = 0
    for i in range(n):
        a, size, want = g["in_%d" % i], tuple(int(v) for v in g["size_%d" % i]), g["out_%d" % i]
        one_axis += (size[0] == a.shape[1]) != (size[1] == a.shape[0])
        got = dev_resize(a, size)
        assert got.shape == want.shape and np.array_equal(got, want), (i, a.shape, size, int((got != want).sum()))
    assert one_axis >= 2


# the issue's full frames, and one whose horizontal table (ksize 401) is too large to be staged in LDS
FULL_FRAMES = [((1600, 900), (400, 225)), ((1226, 370), (613, 185)), ((1241, 376), (480, 302)), ((1600, 900), (1599, 899)),
               ((640, 360), (1226, 370)), ((1600, 900), (384, 384)), ((1600, 900), (8, 5))]


@pytest.mark.parametrize("content", ["random", "bands"])
@pytest.mark.parametrize("src_size,size", FULL_FRAMES)
def test_full_frames(src_size, size, content):
    rng = np.random.default_rng(21 if content == "random" else 22)
    a = R.random_frame(rng, *src_size) if content == "random" else R.banded_frame(rng, *src_size)
    got = dev_resize(a, size)
    want = R.resize(a, size)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    Image = _pil_image()
    if Image is not None:
        assert np.array_equal(got, np.asarray(Image.fromarray(a).resize(size, Image.BILINEAR)))


def test_same_size_returns_the_input():
    dev = torch.zeros((23, 40, 3), dtype=torch.uint8, device="cuda")
    assert spf.resize_bilinear_u8(dev, (40, 23)) is dev
    with pytest.raises(ValueError):
        spf.resize_bilinear_u8(dev, (0, 23))
    with pytest.raises(ValueError):
        spf.resize_bilinear_u8(dev.permute(1, 0, 2), (20, 10))            # pixels of a row are not adjacent
    with pytest.raises(ValueError):
        spf.resize_bilinear_u8(dev.float(), (20, 10))


@pytest.mark.parametrize("size", [(160, 101), (480, 101), (160, 302)])
def test_crop_views_at_every_alignment(size):
    """A view image[top:bottom, left:right] of a frame whose row pitch is odd (3 * 1241 bytes): the row starts take every byte
    alignment.  Both axes, the height alone (the vertical pass reads the view) and the width alone."""
    rng = np.random.default_rng(23)
    base = R.random_frame(rng, 1241, 376)
    dev = torch.from_numpy(base).cuda()
    seen = set()
    top = 74
    for left in range(8):
        view = dev[top:top + 302, left:left + 480]
        assert not view.is_contiguous() and view.stride(0) == 3 * 1241
        seen.add(view.data_ptr() & 3)
        got = spf.resize_bilinear_u8(view, size)
        want = spf.resize_bilinear_u8(view.contiguous(), size)
        assert got.is_contiguous() and torch.equal(got, want), (left, int((got != want).sum()))
        if left in (0, 5):
            assert np.array_equal(got.cpu().numpy(), R.resize(base[top:top + 302, left:left + 480], size)), left
    assert seen == {0, 1, 2, 3}
    # a view that ends on the allocation's last byte
    view = dev[376 - 302:, 1241 - 480:]
    assert torch.equal(spf.resize_bilinear_u8(view, size), spf.resize_bilinear_u8(view.contiguous(), size))


def _jitter_u8(img_u8, draws):
    """torchvision 0.8.2's ColorJitter on a PIL image where Pillow is importable; otherwise the device op, which
    tests/test_color_jitter_gpu.py pins against Pillow."""
    Image = _pil_image()
    if Image is None:
        return spf.color_jitter_u8(torch.from_numpy(img_u8).cuda(), draws).cpu().numpy()
    from tests.test_color_jitter_gpu import pil_jitter
    return pil_jitter(img_u8, draws)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_augment_image_u8_matches_the_nuscenes_loader(dtype):
    """nuscenes_dataloader.py:175-212 restated: rescale the points, resize, truncate to int64, jitter, / 255, flip with the column
    update, normalise, HWC -> CHW."""
    rng = np.random.default_rng(24)
    W, H, n = 1600, 900, 5000
    resize = (400, 225)
    image = R.banded_frame(rng, W, H)
    points_img = np.stack([rng.uniform(0, H, n), rng.uniform(0, W, n)], 1).astype(dtype)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    jitter = draw_color_jitter(0.4, 0.4, 0.4, 0.1, generator=torch.Generator().manual_seed(25))
    assert len(jitter) == 4

    pi = points_img.copy()
    pi[:, 0] = float(resize[1]) / H * np.floor(pi[:, 0])
    pi[:, 1] = float(resize[0]) / W * np.floor(pi[:, 1])
    img = R.resize(image, resize)
    Image = _pil_image()
    if Image is not None:
        assert np.array_equal(img, np.asarray(Image.fromarray(image).resize(resize, Image.BILINEAR)))
    idx = pi.astype(np.int64)
    assert idx.min() >= 0 and idx[:, 0].max() < resize[1] and idx[:, 1].max() < resize[0]
    img = _jitter_u8(img, jitter)
    img = np.array(img, dtype=np.float32) / 255.
    img = np.ascontiguousarray(np.fliplr(img))
    idx[:, 1] = img.shape[1] - 1 - idx[:, 1]
    img = (img - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    want = np.moveaxis(img, -1, 0)

    dev_img, dev_pts = torch.from_numpy(image).cuda(), torch.from_numpy(points_img).cuda()
    got_img, got_idx, got_keep = augment_image_u8(dev_img, dev_pts, None, True, (mean, std), jitter, resize=resize)
    assert got_keep.all() and got_idx.dtype == torch.int64 and np.array_equal(got_idx.cpu().numpy(), idx)
    assert got_img.shape == want.shape and np.array_equal(got_img.cpu().numpy(), want)
    assert np.array_equal(resize_points_img(dev_pts, (W, H), resize).cpu().numpy(), pi)
    # a frame that already has the size goes through untouched, points included
    small = torch.from_numpy(R.random_frame(rng, 400, 225)).cuda()
    a = augment_image_u8(small, dev_pts, None, True, (mean, std), jitter, resize=resize)
    b = augment_image_u8(small, dev_pts, None, True, (mean, std), jitter)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="enlarge"):
        augment_image_u8(small, dev_pts, resize=(1600, 900))


def test_resize_none_is_todays_path():
    """The arguments of test_augment_image_u8_matches_the_dataloader_statements, called with and without the new keyword."""
    from fusiontransformer_amd.data.augment import draw_augmentation_2d
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
        a = augment_image_u8(dev_img, dev_pts, box, flip, (mean, std), jitter)
        b = augment_image_u8(dev_img, dev_pts, box, flip, (mean, std), jitter, resize=None)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), seed


def test_crop_counts_in_the_resized_frame():
    """resize and box together (no reference loader does that): the box is taken from the resized frame."""
    rng = np.random.default_rng(26)
    image = R.random_frame(rng, 1226, 370)
    pts = torch.from_numpy(np.stack([rng.uniform(0, 370, 3000), rng.uniform(0, 1226, 3000)], 1).astype(np.float32)).cuda()
    dev = torch.from_numpy(image).cuda()
    size, box = (613, 185), (100, 35, 580, 185)
    got = augment_image_u8(dev, pts, box, False, None, None, resize=size)
    want = augment_image_u8(spf.resize_bilinear_u8(dev, size), resize_points_img(pts, (1226, 370), size), box, False, None, None)
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and got[0].shape == (3, 150, 480)


def test_steady_state_does_not_synchronise_and_reuses_the_tables():
    rng = np.random.default_rng(27)
    dev = torch.from_numpy(R.random_frame(rng, 1600, 900)).cuda()
    batch = torch.from_numpy(rng.integers(0, 256, (2, 90, 160, 3), dtype=np.uint8)).cuda()
    first = spf.resize_bilinear_u8(dev, (400, 225))                       # first call: table upload, scratch allocation
    spf.resize_bilinear_u8(batch, (40, 23))
    tx, ty = spf.resize_table(1600, 400, dev.device), spf.resize_table(900, 225, dev.device)
    assert tx[0].is_cuda and tx[0].dtype == torch.int32 and tuple(tx[1].shape) == (400, 9) and tx[2] == 9
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = spf.resize_bilinear_u8(dev, (400, 225))
        spf.resize_bilinear_u8(batch, (40, 23))
        spf.resize_bilinear_u8(dev, (400, 900))
        t2 = spf.resize_table(1600, 400, dev.device), spf.resize_table(900, 225, dev.device)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    for old, new in zip((tx, ty), t2):
        assert old[0] is new[0] and old[1] is new[1] and old[2] == new[2]
    assert torch.equal(first, again)                                      # run to run: the same bytes


def test_batch_of_four_equals_four_single_frames():
    rng = np.random.default_rng(28)
    batch = torch.from_numpy(rng.integers(0, 256, (4, 900, 1600, 3), dtype=np.uint8)).cuda()
    got = spf.resize_bilinear_u8(batch, (400, 225))
    assert tuple(got.shape) == (4, 225, 400, 3) and got.is_contiguous()
    for i in range(4):
        assert torch.equal(got[i], spf.resize_bilinear_u8(batch[i], (400, 225))), i
    assert torch.equal(got, spf.resize_bilinear_u8(batch, (400, 225)))
    assert np.array_equal(got[3].cpu().numpy(), R.resize(batch[3].cpu().numpy(), (400, 225)))
    # a batch of crop views: frame stride and row pitch both differ from the packed ones
    views = batch[:, 100:800, 3:1403]
    assert torch.equal(spf.resize_bilinear_u8(views, (350, 175)), spf.resize_bilinear_u8(views.contiguous(), (350, 175)))


_REPLAY_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from fusiontransformer_amd import functional as spf
g = torch.Generator(device="cuda").manual_seed(29)
static_in = torch.randint(0, 256, (4, 900, 1600, 3), device="cuda", generator=g).to(torch.uint8)
other = torch.randint(0, 256, (4, 900, 1600, 3), device="cuda", generator=g).to(torch.uint8)
eager = spf.resize_bilinear_u8(static_in, (400, 225))           # warms the table cache: a capture cannot upload
eager_other = spf.resize_bilinear_u8(other, (400, 225))
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    spf.resize_bilinear_u8(static_in, (400, 225))
torch.cuda.current_stream().wait_stream(side)
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    static_out = spf.resize_bilinear_u8(static_in, (400, 225))
graph.replay()
torch.cuda.synchronize()
assert torch.equal(static_out, eager), "replay differs from the eager launch"
static_in.copy_(other)
graph.replay()
torch.cuda.synchronize()
assert torch.equal(static_out, eager_other), "replay on new contents differs from the eager launch"
print("replay ok")
"""


def test_graph_replay_equals_eager():
    """With the tables cached the call is capturable (its workspace then comes from the graph's pool).  Captured in a fresh process,
    as tests/test_vit_linear_bf16_gpu.py does, so nothing left behind by earlier tests is released while the capture is open."""
    res = subprocess.run([sys.executable, "-c", _REPLAY_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "replay ok" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
