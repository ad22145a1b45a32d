"""Numpy restatement of Pillow's 8-bit bilinear resample (libImaging/Resample.c; the specification in include/ftx.h): the coefficient
table of one axis in Python floats (C doubles), and the two integer passes.  Shared by tests/test_resize_host.py and
tests/test_resize_gpu.py; tests/golden/make_resize_golden.py checks it against Pillow itself when it writes the fixture."""
import ctypes
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2

# (input (width, height), output (width, height)): the NuScenes resize, half-size KITTI, one pixel less, the KITTI crop size from a full
# frame, an enlargement, a tiny frame, a change of aspect ratio
SIZE_PAIRS = [((1600, 900), (400, 225)), ((1226, 370), (613, 185)), ((1600, 900), (1599, 899)), ((1241, 376), (480, 302)),
              ((640, 360), (1226, 370)), ((37, 23), (11, 7)), ((1600, 900), (384, 384))]


def coeffs(in_size, out_size):
    """(bounds (out, 2) int32 = (xmin, taps), kk (out, ksize) int32) of one axis, over the whole axis."""
    in0, in1 = 0.0, float(in_size)
    scale = filterscale = (in1 - in0) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = [0.0] * ksize
        ww = 0.0
        for x in range(xmax):
            a = (x + xmin - center + 0.5) * ss
            if a < 0.0:
                a = -a
            w = 1.0 - a if a < 1.0 else 0.0
            k[x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        for x in range(ksize):
            kk[xx, x] = int(-0.5 + k[x] * (1 << PRECISION_BITS)) if k[x] < 0 else int(0.5 + k[x] * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def library_coeffs(lib):
    """The same table from libftx's host entry points, as a function to pass to `resize(table=...)`."""
    def table(in_size, out_size):
        ksize = lib.ftx_resize_ksize(in_size, out_size)
        assert ksize > 0, lib.ftx_last_error()
        bounds = np.full((out_size, 2), -7, np.int32)
        kk = np.full((out_size, ksize), -7, np.int32)
        vp = ctypes.c_void_p
        assert lib.ftx_resize_coeffs_host(in_size, out_size, bounds.ctypes.data_as(vp), kk.ctypes.data_as(vp)) == 0, lib.ftx_last_error()
        return bounds, kk
    return table


def clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, size, table=coeffs):
    """img (H, W, C) uint8, size = (width, height): horizontal pass into uint8, then the vertical pass on it; a pass whose axis keeps
    its length is skipped.  The sums are below 2^31 (the weights of a tap row add up to about 2^22), so int64 here equals C's int."""
    h, w, c = img.shape
    ow, oh = size
    x = img
    if ow != w:
        b, kk = table(w, ow)
        out = np.empty((h, ow, c), np.uint8)
        for xx in range(ow):
            lo, n = (int(v) for v in b[xx])
            acc = (x[:, lo:lo + n, :].astype(np.int64) * kk[xx, :n].astype(np.int64)[None, :, None]).sum(1) + (1 << (PRECISION_BITS - 1))
            out[:, xx, :] = clip8(acc)
        x = out
    if oh != h:
        b, kk = table(h, oh)
        out = np.empty((oh, x.shape[1], c), np.uint8)
        for yy in range(oh):
            lo, n = (int(v) for v in b[yy])
            acc = (x[lo:lo + n].astype(np.int64) * kk[yy, :n].astype(np.int64)[:, None, None]).sum(0) + (1 << (PRECISION_BITS - 1))
            out[yy] = clip8(acc)
        x = out
    return x


def random_frame(rng, w, h):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def banded_frame(rng, w, h):
    """Random content with saturated bands, a one-pixel column checkerboard, a one-pixel row checkerboard and a one-pixel 2-D
    checkerboard: they reach the clamp and the rounding edge."""
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    s = max(1, h // 9)
    a[0 * s:1 * s] = 255
    a[1 * s:2 * s] = 0
    a[2 * s:3 * s, ::2] = 255
    a[2 * s:3 * s, 1::2] = 0
    a[3 * s:4 * s:2] = 255
    a[3 * s + 1:4 * s:2] = 0
    yy, xx = np.mgrid[4 * s:5 * s, 0:w]
    a[4 * s:5 * s] = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None]
    return a
