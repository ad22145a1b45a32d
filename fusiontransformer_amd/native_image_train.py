"""Host side of the native training executor of the ViT image branch (include/ftx.h: ftx_vit_train_fwd / ftx_vit_train_bwd).

A trunk segment -- blocks [first, last] from one materialised token tensor to the next, what transformers._TrunkSegment runs behind
the embedding -- is ONE autograd node (`_VitSegment`): its forward is one library call, its backward one library call that walks the
blocks in reverse and issues what the per-op nodes of functional.py issue, so the results have that path's bits.  The block table and
the modes are native_image's; the gradient table is written per backward, over one fresh flat buffer per segment.  Everything the
backward reads lives in one arena per forward, allocated from torch's allocator, held by the node and freed when the graph dies.
Nothing is captured, nothing is kept per shape, and an eager pass before it is no obstacle."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from . import functional as spf
from . import native_image as ni
from .native_image import BLOCK, BLOCK_FIELDS, MODEL, Unsupported, _ptr
from .models.transformers import block_switches

# Where the gradients of one block lie in the segment's flat buffer.  ftx_add_layernorm_bwd writes (d gamma, d beta, d y_bias) as one
# array, so norm2_w, norm2_b, proj_b are consecutive, and so are norm1_w, norm1_b and the fc2_b of the block in front (its bias is
# norm1's y_bias); the fc2_b of the segment's last block comes at the very end.
_ORDER = ("qkv_w", "qkv_b", "proj_w", "fc1_w", "fc1_b", "fc2_w", "norm2_w", "norm2_b", "proj_b", "norm1_w", "norm1_b")


def check_record_sizes():
    ni.check_record_sizes()
    assert int(_lib.load().ftx_vit_train_block_bytes()) == BLOCK.itemsize


def arena_bytes(model, n_blocks, first, last, b) -> int:
    """ftx_vit_train_arena_bytes (host only); raises with the library's text for a record or a range it refuses."""
    L = _lib.load()
    n = int(L.ftx_vit_train_arena_bytes(_ptr(model), int(n_blocks), int(first), int(last), int(b)))
    if n == 0:
        raise RuntimeError("ftx_vit_train_arena_bytes: " + L.ftx_last_error().decode("utf-8", "replace"))
    return n


def model_record(bb, tokens):
    """The model record of the trunk `bb` for `tokens` tokens per frame: the sizes only, the executor reads no embedding parameter."""
    t0 = bb.num_tokens
    grid = math.isqrt(max(tokens - t0, 0))
    if grid < 1 or grid * grid != tokens - t0:
        raise Unsupported("%d tokens are not %d + a square grid" % (tokens, t0))
    blk0 = bb.blocks[0]
    model = np.zeros(1, dtype=MODEL)
    m = model[0]
    m["dim"], m["heads"], m["hidden"], m["grid"], m["t0"] = bb.embed_dim, blk0.attn.num_heads, blk0.mlp.fc1.out_features, grid, t0
    m["patch"], m["in_chans"], m["eps"] = bb.patch_embed.patch_size[0], bb.patch_embed.proj.in_channels, blk0.norm1.eps
    return model


def grad_layout(first, last, dim, hidden):
    """({(block, field): (offset, shape)}, total) in floats: the gradients of blocks [first, last] in one flat buffer (see _ORDER)."""
    shapes = dict(norm1_w=(dim,), norm1_b=(dim,), qkv_w=(3 * dim, dim), qkv_b=(3 * dim,), proj_w=(dim, dim), proj_b=(dim,), norm2_w=(dim,),
                  norm2_b=(dim,), fc1_w=(hidden, dim), fc1_b=(hidden,), fc2_w=(dim, hidden), fc2_b=(dim,))
    where, off = {}, 0

    def put(i, f):
        nonlocal off
        where[(i, f)] = (off, shapes[f])
        off += int(np.prod(shapes[f]))

    for i in range(first, last + 1):
        for f in _ORDER:
            put(i, f)
        if i > first:
            put(i - 1, "fc2_b")
    put(last, "fc2_b")
    return where, off


class _Arena:
    """The arena of one forward; the library's note about it goes when the arena goes."""

    def __init__(self, buf):
        self.buf = buf

    def __del__(self):
        try:
            _lib.load().ftx_vit_train_release(self.buf.data_ptr())
        except Exception:      # interpreter shutdown: the library may be gone
            pass


class NativeImageTrain:
    """Per-trunk state of the training executor: the block table with the modes it was written for, rebuilt when a parameter moved or
    a block's execution flags changed.  Runs are per forward and per segment."""

    def __init__(self, trunk):
        check_record_sizes()
        self.trunk = trunk
        self.key = None
        self.tables = None      # (blocks, keep, linear_mode, attn_mode) or the Unsupported that refused the trunk
        self.models = {}        # tokens per frame -> model record
        self.runs = 0           # segments this executor ran (the tests' witness)
        self.last_arena_bytes = 0

    def live(self):
        bb = self.trunk
        return bb.blocks[:len(bb.blocks) if bb.last_block is None else bb.last_block + 1]

    def _signature(self):
        sig = []
        for blk in self.live():
            sig.extend(t.data_ptr() for t in ni.block_tensors(blk))
            sig.append(block_switches(blk))
        return tuple(sig)

    def ready(self):
        """(blocks, keep, linear_mode, attn_mode) for the trunk as it is now; raises Unsupported (every time, with the reason)."""
        key = self._signature()
        if key != self.key:
            self.key, self.tables, self.models = key, None, {}
            try:
                modes = ni.trunk_modes(self.trunk)      # first: a trunk the executor does not run builds nothing
                keep = []
                self.tables = (ni.block_table(self.trunk, ni.keeper(keep)), keep) + modes
            except Unsupported as err:
                self.tables = err
        if isinstance(self.tables, Unsupported):
            raise self.tables
        return self.tables

    def model(self, tokens):
        m = self.models.get(tokens)
        if m is None:
            m = self.models[tokens] = model_record(self.trunk, tokens)
        return m

    def segment(self, x, first, last):
        """Blocks [first, last] on the tokens x (b, T, dim) as one autograd node."""
        params = [t for blk in self.live()[first:last + 1] for t in ni.block_tensors(blk)]
        return _VitSegment.apply(self, first, last, x, *params)


class _VitSegment(torch.autograd.Function):
    """(executor, first, last, tokens, *the twelve parameters of every block of the segment) -> tokens."""

    @staticmethod
    def forward(ctx, ex, first, last, x, *params):
        blocks, _, linear_mode, attn_mode = ex.tables if isinstance(ex.tables, tuple) else ex.ready()
        x = _lib.req(x.contiguous(), torch.float32, "native image train tokens", 3)
        b, tokens, dim = x.shape
        model = ex.model(tokens)
        if dim != int(model[0]["dim"]) or len(params) != 12 * (last - first + 1):
            raise ValueError("native image train: the tokens or the parameters do not match the trunk")
        need = arena_bytes(model, len(blocks), first, last, b)
        buf = torch.empty((need,), dtype=torch.uint8, device=x.device)
        out = torch.empty_like(x)
        L = _lib.load()
        spf._log_launch("vit_train_fwd", dict(b=b, first=first, last=last, linear_mode=linear_mode, attn_mode=attn_mode), lambda: _lib.check(
            L.ftx_vit_train_fwd(_ptr(model), _ptr(blocks), len(blocks), b, x.data_ptr(), first, last, linear_mode, attn_mode, out.data_ptr(),
                                buf.data_ptr(), need, _lib.stream()), "ftx_vit_train_fwd"))
        ex.runs += 1
        ex.last_arena_bytes = need
        ctx.call = (model, blocks, linear_mode, attn_mode, first, last)
        ctx.arena = _Arena(buf)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.arena is None:
            raise RuntimeError("native image train: this segment has given its gradients; the backward overwrites what the forward kept, so a second "
                               "backward needs a second forward")
        (x,) = ctx.saved_tensors
        model, blocks, linear_mode, attn_mode, first, last = ctx.call
        arena, ctx.arena = ctx.arena, None      # whatever happens below, this run is consumed from here
        grad_out = _lib.req(grad_out.contiguous(), torch.float32, "native image train output gradient", 3)
        if grad_out.shape != x.shape:
            raise ValueError("native image train: the output gradient does not match the tokens")
        m = model[0]
        where, total = grad_layout(first, last, int(m["dim"]), int(m["hidden"]))
        flat = torch.empty((total,), dtype=torch.float32, device=x.device)
        base = flat.data_ptr()
        grads = np.zeros(len(blocks), dtype=BLOCK)
        for (i, f), (off, _) in where.items():
            grads[i][f] = base + 4 * off
        grad_in = torch.empty_like(x)
        b = x.shape[0]
        L = _lib.load()
        spf._log_launch("vit_train_bwd", dict(b=b, first=first, last=last, linear_mode=linear_mode, attn_mode=attn_mode), lambda: _lib.check(
            L.ftx_vit_train_bwd(_ptr(model), _ptr(blocks), _ptr(grads), len(blocks), b, x.data_ptr(), grad_out.data_ptr(), first, last, linear_mode,
                                attn_mode, grad_in.data_ptr(), arena.buf.data_ptr(), arena.buf.shape[0], _lib.stream()), "ftx_vit_train_bwd"))
        out = []
        for i in range(first, last + 1):
            for f in BLOCK_FIELDS:
                off, shape = where[(i, f)]
                out.append(flat[off:off + int(np.prod(shape))].view(shape))
        return (None, None, None, grad_in, *out)
