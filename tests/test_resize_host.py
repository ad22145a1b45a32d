"""Image resize on the host: libftx's coefficient table (ftx_resize_coeffs_host, no GPU needed) against the numpy restatement of
Pillow's Resample.c, the restatement driven by that table against Pillow itself where it is importable, the rule that rescales the
projected points against numpy's two statements, and the C-ABI argument checks (nothing is launched).  Every comparison is equality."""
import ctypes

import numpy as np
import pytest
import torch

from fusiontransformer_amd.data.augment import augment_image_u8, resize_points_img
from tests import resize_ref as R


def axis_pairs():
    pairs = set()
    for (w, h), (ow, oh) in R.SIZE_PAIRS:
        pairs.add((w, ow))
        pairs.add((h, oh))
    pairs |= {(900, 900), (1600, 1), (900, 1), (1, 400), (1, 1), (1600, 8)}
    pairs |= {(i, o) for i in range(1, 49) for o in range(1, 49)}
    return sorted(pairs)


def test_library_table_equals_the_restatement(ftx_lib):
    table = R.library_coeffs(ftx_lib)
    pairs = axis_pairs()
    assert len(pairs) > 48 * 48
    for in_size, out_size in pairs:
        want_b, want_k = R.coeffs(in_size, out_size)
        assert ftx_lib.ftx_resize_ksize(in_size, out_size) == want_k.shape[1], (in_size, out_size)
        got_b, got_k = table(in_size, out_size)
        assert np.array_equal(got_b, want_b), (in_size, out_size)
        assert np.array_equal(got_k, want_k), (in_size, out_size)
        # what the kernels rely on: every tap inside the axis and the table, weights that fit a 24-bit multiply
        assert (got_b[:, 0] >= 0).all() and (got_b[:, 1] >= 1).all() and (got_b.sum(1) <= in_size).all() and (got_b[:, 1] <= got_k.shape[1]).all()
        assert got_k.min() >= 0 and got_k.max() <= 1 << R.PRECISION_BITS


def test_same_length_table_is_the_identity(ftx_lib):
    """in == out: taps (xx, xx + 1) with weights (1, 0); Pillow skips such a pass, and running it would change nothing."""
    b, k = R.library_coeffs(ftx_lib)(37, 37)
    assert k.shape == (37, 3) and (k[:, 0] == 1 << R.PRECISION_BITS).all() and (k[:, 1:] == 0).all()
    assert np.array_equal(b[:, 0], np.arange(37))


@pytest.mark.parametrize("content", ["random", "bands"])
def test_restatement_on_library_tables_equals_pillow(ftx_lib, content):
    Image = pytest.importorskip("PIL.Image")
    table = R.library_coeffs(ftx_lib)
    rng = np.random.default_rng(11 if content == "random" else 12)
    for (w, h), size in R.SIZE_PAIRS:
        a = R.random_frame(rng, w, h) if content == "random" else R.banded_frame(rng, w, h)
        want = np.asarray(Image.fromarray(a).resize(size, Image.BILINEAR))
        got = R.resize(a, size, table)
        assert got.shape == want.shape and np.array_equal(got, want), ((w, h), size, int((got != want).sum()))


def test_restatement_equals_pillow_on_small_frames(ftx_lib):
    """Every pair of widths in 1..24, 47, 48, heights varied alongside, `in == 1` and `out == 1` included."""
    Image = pytest.importorskip("PIL.Image")
    table = R.library_coeffs(ftx_lib)
    rng = np.random.default_rng(13)
    sizes = list(range(1, 25)) + [47, 48]
    for i, w in enumerate(sizes):
        for j, ow in enumerate(sizes):
            h, oh = sizes[(i * 7 + j) % len(sizes)], sizes[(i + j * 5 + 3) % len(sizes)]
            a = R.random_frame(rng, w, h)
            want = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))
            assert np.array_equal(R.resize(a, (ow, oh), table), want), ((w, h), (ow, oh))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("image_size,resize", [((1600, 900), (400, 225)), ((1226, 370), (480, 302)), ((1241, 376), (613, 185))])
def test_resize_points_img_follows_numpy(dtype, image_size, resize):
    """nuscenes_dataloader.py:181-182 as written, on 200 000 points: ratios 225/900 and 400/1600 (dyadic), 302/370, 480/1226, 185/376,
    613/1241 (not)."""
    rng = np.random.default_rng(14)
    n = 200000
    points_img = np.stack([rng.uniform(0, image_size[1], n), rng.uniform(0, image_size[0], n)], 1).astype(dtype)
    want = points_img.copy()
    want[:, 0] = float(resize[1]) / image_size[1] * np.floor(want[:, 0])
    want[:, 1] = float(resize[0]) / image_size[0] * np.floor(want[:, 1])
    got = resize_points_img(torch.from_numpy(points_img), image_size, resize)
    assert got.dtype == torch.from_numpy(points_img).dtype and np.array_equal(got.numpy(), want)
    assert np.array_equal(got.to(torch.int64).numpy(), want.astype(np.int64))
    if dtype == np.float32 and image_size == (1226, 370):
        # the rule is not "float64 product, rounded to float32"
        other = (np.float64(float(resize[1]) / image_size[1]) * np.floor(points_img[:, 0]).astype(np.float64)).astype(np.float32)
        assert (other != want[:, 0]).any()


def test_resize_points_img_rejects_other_inputs():
    with pytest.raises(ValueError):
        resize_points_img(torch.zeros((4, 2), dtype=torch.int64), (1600, 900), (400, 225))
    with pytest.raises(ValueError):
        resize_points_img(torch.zeros((4, 3)), (1600, 900), (400, 225))


def test_augment_image_u8_refuses_to_enlarge():
    """The loader's `assert image.size[0] > self.resize[0]`, raised before anything touches the device."""
    with pytest.raises(ValueError, match="enlarge"):
        augment_image_u8(torch.zeros((90, 160, 3), dtype=torch.uint8), torch.zeros((1, 2)), resize=(320, 180))


def _call(lib, src=4096, frame_stride=0, pitch=480, n=1, in_h=90, in_w=160, c=3, bx=4096, kx=4096, ksx=None, by=4096, ky=4096, ksy=None,
          out_h=23, out_w=40, dst=4096, ws=4096, ws_bytes=None):
    """Pointers are never dereferenced: every call below is refused on the host (or has nothing to do)."""
    ksx = lib.ftx_resize_ksize(in_w, out_w) if ksx is None else ksx
    ksy = lib.ftx_resize_ksize(in_h, out_h) if ksy is None else ksy
    ws_bytes = lib.ftx_resize_workspace_bytes(n, in_h, in_w, out_h, out_w) if ws_bytes is None else ws_bytes
    return lib.ftx_resize_bilinear_u8(src, frame_stride, pitch, n, in_h, in_w, c, bx, kx, ksx, by, ky, ksy, out_h, out_w, dst, ws, ws_bytes, None)


def test_cabi_rejects_bad_arguments_before_launching(ftx_lib):
    L = ftx_lib
    buf = (ctypes.c_int32 * 64)()
    for args in ((0, 4, buf, buf), (4, 0, buf, buf), (-3, 4, buf, buf)):
        assert L.ftx_resize_coeffs_host(*args) == -1 and b"positive" in L.ftx_last_error(), args
    assert L.ftx_resize_coeffs_host(8, 4, None, buf) == -1 and b"null pointer" in L.ftx_last_error()
    assert L.ftx_resize_coeffs_host(8, 4, buf, None) == -1 and b"null pointer" in L.ftx_last_error()
    assert L.ftx_resize_ksize(0, 4) == -1 and b"positive" in L.ftx_last_error()
    assert L.ftx_resize_ksize(4, -1) == -1 and b"positive" in L.ftx_last_error()
    assert L.ftx_resize_ksize(1600, 400) == 9 and L.ftx_resize_ksize(900, 225) == 9 and L.ftx_resize_ksize(360, 370) == 3

    # the workspace is a pure function of the arguments: the padded uint8 intermediate when both axes change, nothing otherwise
    assert L.ftx_resize_workspace_bytes(4, 900, 1600, 225, 400) == 4 * 900 * 1200
    assert L.ftx_resize_workspace_bytes(1, 90, 161, 23, 41) == 90 * 12 * 11
    assert L.ftx_resize_workspace_bytes(1, 900, 1600, 900, 400) == 0 and L.ftx_resize_workspace_bytes(1, 900, 1600, 225, 1600) == 0
    assert L.ftx_resize_workspace_bytes(0, 900, 1600, 225, 400) == 0 and L.ftx_resize_workspace_bytes(1, -1, 1600, 225, 400) == 0

    cases = [
        (dict(n=-1), b"n_frames"),
        (dict(in_h=0), b"positive"),
        (dict(out_w=0), b"positive"),
        (dict(c=4), b"channels"),
        (dict(pitch=479), b"pitch"),
        (dict(frame_stride=-480), b"frame stride"),
        (dict(out_h=90, out_w=160), b"nothing to resample"),
        (dict(bx=None), b"horizontal table"),
        (dict(ky=None), b"vertical table"),
        (dict(ksx=5), b"ksize_x"),
        (dict(ksy=11), b"ksize_y"),
        (dict(src=None), b"null pointer"),
        (dict(dst=None), b"null pointer"),
        (dict(ws=None), b"workspace"),
        (dict(ws_bytes=90 * 120 - 1), b"workspace"),
        (dict(ws=4100), b"16-byte aligned"),
    ]
    for kw, msg in cases:
        assert _call(L, **kw) == -1, kw
        assert msg in L.ftx_last_error(), (kw, L.ftx_last_error())
    assert _call(L, n=0) == 0                                            # no frames: a no-op
