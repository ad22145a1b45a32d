"""Colour jitter on the host: the draws (torchvision 0.8.2 ColorJitter restated), the C-ABI argument checks (nothing is launched),
and the uint8 rules the kernel implements (csrc/ftx_image_ops.h) checked exhaustively against Pillow where it is importable."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from fusiontransformer_amd.data.augment import draw_color_jitter

NAMES = ("brightness", "contrast", "saturation", "hue")


def torchvision_forward_draws(ranges, g):
    """torchvision 0.8.2 ColorJitter.forward, with the image calls replaced by recording (op, factor)."""
    fn_idx = torch.randperm(4, generator=g)
    out = []
    for fn_id in fn_idx:
        if fn_id == 0 and ranges[0] is not None:
            out.append(("brightness", torch.tensor(1.0).uniform_(ranges[0][0], ranges[0][1], generator=g).item()))
        if fn_id == 1 and ranges[1] is not None:
            out.append(("contrast", torch.tensor(1.0).uniform_(ranges[1][0], ranges[1][1], generator=g).item()))
        if fn_id == 2 and ranges[2] is not None:
            out.append(("saturation", torch.tensor(1.0).uniform_(ranges[2][0], ranges[2][1], generator=g).item()))
        if fn_id == 3 and ranges[3] is not None:
            out.append(("hue", torch.tensor(1.0).uniform_(ranges[3][0], ranges[3][1], generator=g).item()))
    return out


@pytest.mark.parametrize("cfg,ranges", [
    ((0.4, 0.4, 0.4), [[0.6, 1.4], [0.6, 1.4], [0.6, 1.4], None]),
    ((0.4, 0.4, 0.4, 0.1), [[0.6, 1.4], [0.6, 1.4], [0.6, 1.4], [-0.1, 0.1]]),
    ((1.5, 0, (0.2, 2.0), (-0.5, 0.25)), [[0.0, 2.5], None, [0.2, 2.0], [-0.5, 0.25]]),
    ((0, 0.3), [None, [0.7, 1.3], None, None]),
])
def test_draws_follow_torchvision_0_8_2(cfg, ranges):
    for seed in range(20):
        got = draw_color_jitter(*cfg, generator=torch.Generator().manual_seed(seed))
        want = torchvision_forward_draws(ranges, torch.Generator().manual_seed(seed))
        assert got == want, (cfg, seed)
    # the global generator when none is given
    torch.manual_seed(5)
    got = draw_color_jitter(*cfg)
    torch.manual_seed(5)
    assert got == torchvision_forward_draws(ranges, None)


def test_off_ops_and_errors():
    assert draw_color_jitter() == []
    assert draw_color_jitter(0, (1, 1), 0, (0, 0)) == []
    assert [op for op, _ in draw_color_jitter(0, 0, 0, 0.2, generator=torch.Generator().manual_seed(1))] == ["hue"]
    with pytest.raises(ValueError, match="non negative"):
        draw_color_jitter(-0.1)
    with pytest.raises(ValueError, match="should be between"):
        draw_color_jitter(0, (1.5, 1.0))
    with pytest.raises(ValueError, match="should be between"):
        draw_color_jitter(0, 0, 0, (-0.6, 0.1))
    with pytest.raises(TypeError):
        draw_color_jitter((0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match="is not in"):      # a hue number above 0.5: adjust_hue refuses the factor it drew
        for seed in range(50):
            draw_color_jitter(0, 0, 0, 4.0, generator=torch.Generator().manual_seed(seed))


def test_numpy_random_state_is_untouched():
    np.random.seed(11)
    before = np.random.get_state()
    for _ in range(10):
        draw_color_jitter(0.4, 0.4, 0.4, 0.1)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def _call_u8(lib, src=None, pitch=30, h=4, w=10, c=3, ops=(0,), factors=(1.0,), n=None, dst=None, ws=None, ws_bytes=0):
    n = len(ops) if n is None else n
    o = (ctypes.c_int32 * max(1, len(ops)))(*ops)
    f = (ctypes.c_double * max(1, len(factors)))(*factors)
    return lib.ftx_color_jitter_u8(src, pitch, h, w, c, o, f, n, dst, ws, ws_bytes, None)


def test_cabi_rejects_bad_arguments_before_launching(ftx_lib):
    L = ftx_lib
    p = ctypes.c_void_p(4096)               # never dereferenced: every call below is refused on the host
    assert L.ftx_color_jitter_workspace_bytes(370, 1226) >= 370 * 1226 * 3
    cases = [
        (dict(src=p, dst=p, ops=(7,)), b"unknown op"),
        (dict(src=p, dst=p, ops=(0, 1, 2, 3, 0), factors=(1,) * 5), b"n_ops"),
        (dict(src=p, dst=p, ops=(2, 2), factors=(1, 1)), b"repeated"),
        (dict(src=p, dst=p, ops=(0,), factors=(-0.5,)), b"negative"),
        (dict(src=p, dst=p, ops=(3,), factors=(0.6,)), b"hue factor"),
        (dict(src=None, dst=p), b"null pointer"),
        (dict(src=p, dst=None), b"null pointer"),
        (dict(src=p, dst=p, pitch=29), b"pitch"),
        (dict(src=p, dst=p, c=4), b"channels"),
        (dict(src=p, dst=p, ops=(1,), ws=None), b"workspace"),
        (dict(src=p, dst=p, ops=(1,), ws=p, ws_bytes=16), b"workspace"),
    ]
    for kw, msg in cases:
        assert _call_u8(L, **kw) == -1, kw
        assert msg in L.ftx_last_error(), (kw, L.ftx_last_error())
    assert _call_u8(L, h=0, src=None, dst=None) == 0           # empty frame: a no-op
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert L.ftx_color_jitter_chw(p, 30, 4, 10, 3, None, None, 0, 0, m, None, p, None, 0, None) == -1
    assert b"mean and std" in L.ftx_last_error()
    z = (ctypes.c_float * 3)(1.0, 0.0, 1.0)
    assert L.ftx_color_jitter_chw(p, 30, 4, 10, 3, None, None, 0, 0, m, z, p, None, 0, None) == -1
    assert b"zero" in L.ftx_last_error()


# ---- the uint8 rules of the kernel (csrc/ftx_image_ops.h), restated in numpy and checked against Pillow on the CPU ----

def blend_rule(in1, in2, alpha):
    """Image.blend: float32(in1) + float32(alpha) * float32(in2 - in1), each operation rounded to float32, truncated, clipped."""
    a = np.float32(alpha)
    t = np.asarray(in1, np.float32) + a * (np.asarray(in2, np.int32) - np.asarray(in1, np.int32)).astype(np.float32)
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def luma_rule(rgb):
    rgb = rgb.astype(np.int64)
    return ((19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 0x8000) >> 16).astype(np.uint8)


def contrast_grey_rule(rgb):
    s = int(luma_rule(rgb).astype(np.int64).sum())
    return int(s / (rgb.shape[0] * rgb.shape[1]) + 0.5)


def all_colours():
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_blend_rule_matches_pillow_for_every_pair():
    Image = pytest.importorskip("PIL.Image")
    a = np.repeat(np.arange(256, dtype=np.uint8), 256).reshape(256, 256)
    b = np.tile(np.arange(256, dtype=np.uint8), 256).reshape(256, 256)
    for alpha in (0.0, 0.3, 0.6, 0.999, 1.0, 1.37, 1.4, 2.5, 3.0):
        want = np.asarray(Image.blend(Image.fromarray(a, "L"), Image.fromarray(b, "L"), alpha))
        assert np.array_equal(blend_rule(a, b, alpha), want), alpha
    # the same expression in double, or with one rounding (a fused multiply-add), is NOT Pillow's
    want = np.asarray(Image.blend(Image.fromarray(a, "L"), Image.fromarray(b, "L"), 1.37))
    exact = a.astype(np.float64) + np.float64(np.float32(1.37)) * (b.astype(np.float64) - a)   # exact in double
    assert (np.clip(np.trunc(exact), 0, 255).astype(np.uint8) != want).sum() == 118
    assert not np.array_equal(np.clip(np.trunc(exact.astype(np.float32)), 0, 255).astype(np.uint8), want)


def test_luma_rule_matches_pillow_on_every_colour():
    Image = pytest.importorskip("PIL.Image")
    img = all_colours()
    assert np.array_equal(luma_rule(img), np.asarray(Image.fromarray(img, "RGB").convert("L")))


def test_contrast_grey_rule_matches_pillow():
    pytest.importorskip("PIL.Image")
    from PIL import Image, ImageEnhance
    rng = np.random.default_rng(0)
    for h, w in itertools.product((1, 7, 64), (1, 33, 96)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        grey = contrast_grey_rule(img)
        got = np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(0.0))   # factor 0: the degenerate image itself
        assert (got == grey).all(), (h, w)
