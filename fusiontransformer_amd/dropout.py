"""The library's counter-based Dropout (include/ftx.h: ftx_dropout / ftx_dropout_mask), published as functional.dropout and
functional.dropout_mask.

The mask is a pure function of (seed, call, logical element index) -- Philox4x32-10, the contract in include/ftx.h, restated in
numpy by tests/dropout_ref.py -- so it is the same on every device and torch version, can be stated after the fact, and is
recomputed in the backward instead of being saved: the node keeps four numbers and no tensor."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, req, stream

U64 = (1 << 64) - 1


def _stream_args(p, seed, call, elem0, who):
    """(p, seed, call, elem0) as the entry takes them, or ValueError: p must lie in [0, 1) AS A FLOAT32, the counters in [0, 2^64)."""
    try:
        p = float(np.float32(p))
    except (TypeError, ValueError):
        raise ValueError(f"{who}: p must be a number in [0, 1)")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{who}: p = {p} outside [0, 1)")
    out = [p]
    for name, v in (("seed", seed), ("call", call), ("elem0", elem0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= U64:
            raise ValueError(f"{who}: {name} must be an integer in [0, 2^64)")
        out.append(int(v))
    return out


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, call, elem0, inplace):
        x = req(x if inplace else x.contiguous(), torch.float32, "dropout x")
        if inplace:
            ctx.mark_dirty(x)
        y = x if inplace else torch.empty_like(x)
        check(_lib.load().ftx_dropout(ptr(x), x.numel(), p, seed, call, elem0, ptr(y), stream()), "ftx_dropout")
        ctx.args = (p, seed, call, elem0)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        grad_out = req(grad_out.contiguous(), torch.float32, "dropout grad")
        gx = torch.empty_like(grad_out)
        check(_lib.load().ftx_dropout(ptr(grad_out), grad_out.numel(), *ctx.args, ptr(gx), stream()), "ftx_dropout")
        return gx, None, None, None, None, None


def dropout(x, p, seed, call, elem0=0, inplace=False):
    """x * mask * float32(1 / (1 - p)) with the mask of (seed, call, elem0 + index into x) (ftx_dropout): one autograd node whose backward
    is the same launch on the gradient.  x: a float32 CUDA tensor of any shape (contiguous when inplace=True, which overwrites it)."""
    p, seed, call, elem0 = _stream_args(p, seed, call, elem0, "dropout")
    if inplace or not isinstance(x, torch.Tensor):      # the node checks device and dtype; in place the tensor itself must be contiguous
        req(x, torch.float32, "dropout x")
    return _Dropout.apply(x, p, seed, call, elem0, bool(inplace))


def dropout_mask(shape, p, seed, call, elem0=0, device="cuda"):
    """The bool keep-mask dropout() applies to a tensor of `shape` for the same (p, seed, call, elem0) (ftx_dropout_mask)."""
    p, seed, call, elem0 = _stream_args(p, seed, call, elem0, "dropout_mask")
    shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
    if any(s < 0 for s in shape):
        raise ValueError("dropout_mask: negative size")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("dropout_mask: expected a CUDA (HIP) device; the product path has no CPU fallback")
    with torch.cuda.device(device):
        keep = torch.empty(shape, dtype=torch.uint8, device=device)
        check(_lib.load().ftx_dropout_mask(keep.numel(), p, seed, call, elem0, ptr(keep), stream()), "ftx_dropout_mask")
    return keep.view(torch.bool)
