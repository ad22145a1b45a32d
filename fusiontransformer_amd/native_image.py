"""Host side of the native eval-mode executor of the ViT image branch (include/ftx.h: ftx_vit_eval).

The trunk is three tables -- one model record, one record per block, one per tap -- that `emit` writes from the module tree of a
Net2DBillinear at the parameters' present addresses.  Per batch the host sizes the arena, allocates the tap outputs and makes one
library call per trunk segment (up to the middle tap, then up to the late tap); everything in between lives in an arena the module
owns, one per (device, stream)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import functional as spf
from .models.transformers import OWN_BF16, OWN_SPLIT, block_linears, block_switches, linear_route, linear_switches

_P = "<i8"   # a device pointer in a table
MODEL = np.dtype([("patch_w", _P), ("patch_b", _P), ("cls", _P), ("dist", _P), ("pos", _P), ("dim", "<i4"), ("heads", "<i4"), ("hidden", "<i4"),
                  ("patch", "<i4"), ("grid", "<i4"), ("t0", "<i4"), ("in_chans", "<i4"), ("eps", "<f4")])
BLOCK_FIELDS = ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
BLOCK = np.dtype([(n, _P) for n in BLOCK_FIELDS])
TAP = np.dtype([("stem_w", _P), ("stem_b", _P), ("gamma", _P), ("beta", _P), ("mean", _P), ("var", _P), ("block", "<i4"), ("co", "<i4"),
                ("eps", "<f4"), ("reserved", "<i4")])
LINEAR_SPLIT, LINEAR_BF16 = 0, 1
ATTN_FP32, ATTN_BF16, ATTN_SPLIT = 0, 1, 2
_ATTN_MODE = {"ftx": ATTN_FP32, "ftx_bf16": ATTN_BF16, "ftx_split": ATTN_SPLIT}
_LINEAR_MODE = {OWN_SPLIT: LINEAR_SPLIT, OWN_BF16: LINEAR_BF16}      # of the routes the executor runs (transformers.linear_route)

_vp = ctypes.c_void_p


def check_record_sizes():
    L = _lib.load()
    assert int(L.ftx_vit_model_bytes()) == MODEL.itemsize and int(L.ftx_vit_block_bytes()) == BLOCK.itemsize
    assert int(L.ftx_vit_tap_bytes()) == TAP.itemsize


class Unsupported(Exception):
    """The module tree holds something the executor does not run; the caller takes the Python path.  The text is the reason."""


def _ptr(a):
    return a.ctypes.data_as(_vp)


def block_tensors(blk):
    """The twelve tensors of a transformers.Block in the block record's order."""
    return (blk.norm1.weight, blk.norm1.bias, blk.attn.qkv.weight, blk.attn.qkv.bias, blk.attn.proj.weight, blk.attn.proj.bias,
            blk.norm2.weight, blk.norm2.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias)


def tap_tensors(up):
    """(stem weight, stem bias, gamma, beta, running_mean, running_var) of a BilinearModule."""
    conv, bn = up.stem[0], up.stem[2]
    return conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var


def trunk_modes(bb):
    """(linear_mode, attn_mode) that every live block of the trunk `bb` (an Image2DTransformer) shares, or Unsupported with the reason."""
    live = [b for i, b in enumerate(bb.blocks) if bb.last_block is None or i <= bb.last_block]
    lin, att = set(), set()
    for blk in live:
        for l in block_linears(blk):
            route = linear_route(l)
            if route not in _LINEAR_MODE:
                impl = linear_switches(l)[0]
                raise Unsupported("vit_linear_impl=%r%s: the library has no GEMM of its own for these Linears" % (
                    impl, "" if impl != "ftx" else " without set_bf16"))
            lin.add(_LINEAR_MODE[route])
        att.add(blk.attn.attn_impl)
    if len(lin) != 1:
        raise Unsupported("the blocks do not share one linear mode")
    if len(att) != 1 or next(iter(att)) not in _ATTN_MODE:
        raise Unsupported("attn_impl %s: the executor runs 'ftx', 'ftx_bf16' or 'ftx_split' on every block" % sorted(att))
    return lin.pop(), _ATTN_MODE[att.pop()]


def modes(net):
    """trunk_modes of a Net2DBillinear's trunk."""
    return trunk_modes(net.backbone)


def _taps_of(net):
    """[(block index, key of net.up)] ascending; the middle tap first when both read the same block."""
    late = int(net.late_feat_block_number)
    taps = [(late, net.late_feat_block_number)]
    mid = net.middle_feat_block_number
    if mid is not None and mid in net.up and int(mid) != late:
        if int(mid) > late:
            raise Unsupported("the middle tap lies behind the late tap")
        taps.insert(0, (int(mid), mid))
    return taps


def block_table(bb, dev):
    """The block records of the live blocks of the trunk `bb` at the parameters' present addresses; dev(tensor, what) -> address keeps
    the tensor.  Raises Unsupported for a block that is not the fused timm block."""
    import torch.nn as nn
    n_live = len(bb.blocks) if bb.last_block is None else bb.last_block + 1
    blk0 = bb.blocks[0]
    blocks = np.zeros(n_live, dtype=BLOCK)
    for i in range(n_live):
        blk = bb.blocks[i]
        act = blk.mlp.act
        if (type(blk.norm1) is not nn.LayerNorm or type(blk.norm2) is not nn.LayerNorm or not isinstance(blk.drop_path, nn.Identity)
                or type(act) is not nn.GELU or act.approximate != "none" or blk.mlp.drop.p != 0.0 or blk.attn.proj_drop.p != 0.0
                or blk.attn.attn_drop.p != 0.0 or blk.norm1.eps != blk0.norm1.eps or blk.norm2.eps != blk0.norm1.eps
                or blk.attn.num_heads != blk0.attn.num_heads or blk.mlp.fc1.out_features != blk0.mlp.fc1.out_features
                or blk.attn.scale != 0.125):
            raise Unsupported("block %d is not the fused timm block (LayerNorm, exact GELU, no dropout, 64-wide heads)" % i)
        for name, t in zip(BLOCK_FIELDS, block_tensors(blk)):
            blocks[i][name] = dev(t, "block %d %s" % (i, name))
    return blocks


def keeper(keep):
    """dev(tensor, what) of block_table / emit: the address of a contiguous float32 tensor, which is appended to `keep`."""
    def dev(t, what):
        if t is None or t.dtype != torch.float32 or not t.is_contiguous():
            raise Unsupported(what + ": parameters must be contiguous float32")
        keep.append(t)
        return t.data_ptr()
    return dev


def emit(net):
    """(model, blocks, taps, keep) of a Net2DBillinear: the three tables at the parameters' present addresses; `keep` holds every tensor
    the tables point to.  Raises Unsupported for a module tree the executor does not run."""
    import torch.nn as nn
    bb = net.backbone
    pe = bb.patch_embed
    conv = pe.proj
    P = pe.patch_size[0]
    if pe.patch_size[0] != pe.patch_size[1] or conv.stride != conv.kernel_size or conv.bias is None or not isinstance(pe.norm, nn.Identity):
        raise Unsupported("patch embedding is not a square Conv2d(kernel = stride) with a bias")
    if bb.pos_drop.p != 0.0:
        raise Unsupported("pos_drop is not the identity")
    dim = bb.embed_dim
    side = net.sample_down.size
    if side[0] != side[1] or side[0] % P:
        raise Unsupported("the resampled image is not a square of whole patches")
    grid = side[0] // P
    t0 = bb.num_tokens
    if tuple(bb.pos_embed.shape) != (1, t0 + grid * grid, dim):
        raise Unsupported("pos_embed does not match the token grid")
    keep = []
    dev = keeper(keep)
    model = np.zeros(1, dtype=MODEL)
    m = model[0]
    m["patch_w"], m["patch_b"], m["cls"], m["pos"] = (dev(t, "patch embedding") for t in (conv.weight, conv.bias, bb.cls_token, bb.pos_embed))
    m["dist"] = dev(bb.dist_token, "dist token") if bb.dist_token is not None else 0
    blk0 = bb.blocks[0]
    m["dim"], m["heads"], m["hidden"], m["patch"], m["grid"], m["t0"], m["in_chans"] = dim, blk0.attn.num_heads, blk0.mlp.fc1.out_features, P, grid, t0, conv.in_channels
    m["eps"] = blk0.norm1.eps
    blocks = block_table(bb, dev)
    spec = _taps_of(net)
    taps = np.zeros(len(spec), dtype=TAP)
    for r, (block, key) in zip(taps, spec):
        up = net.up[key]
        cv, bn = up.stem[0], up.stem[2]
        if cv.in_channels != dim or not bn.track_running_stats or not bn.affine or cv.bias is None:
            raise Unsupported("tap %s: Conv1x1 with a bias -> ReLU -> BatchNorm with running statistics expected" % key)
        r["stem_w"], r["stem_b"], r["gamma"], r["beta"], r["mean"], r["var"] = (dev(t, "tap " + key) for t in tap_tensors(up))
        r["block"], r["co"], r["eps"] = block, cv.out_channels, bn.eps
    return model, blocks, taps, keep


def arena_bytes(model, n_blocks, b) -> int:
    """ftx_vit_eval_arena_bytes (host only); raises with the library's text for a record it refuses."""
    L = _lib.load()
    n = int(L.ftx_vit_eval_arena_bytes(_ptr(model), int(n_blocks), int(b)))
    if n == 0:
        raise RuntimeError("ftx_vit_eval_arena_bytes: " + L.ftx_last_error().decode("utf-8", "replace"))
    return n


def eval_call(model, blocks, taps, b, img, tokens_in, first, last, linear_mode, attn_mode, outs, arena, stream=None):
    """One ftx_vit_eval call: blocks [first, last] with the first `len(outs)` records of `taps`; `outs`: one tensor or None per tap."""
    L = _lib.load()
    ptrs = (_vp * max(1, len(outs)))(*[None if o is None else o.data_ptr() for o in outs])
    _lib.check(L.ftx_vit_eval(_ptr(model), _ptr(blocks), len(blocks), _ptr(taps), len(outs), int(b), _lib.ptr(img), _lib.ptr(tokens_in), int(first),
                              int(last), int(linear_mode), int(attn_mode), ptrs, arena.data_ptr(), arena.shape[0],
                              _lib.stream() if stream is None else stream), "ftx_vit_eval")


class NativeImage:
    """Per-module state of the executor: the tables with the modes they were written for (rebuilt when a parameter moved or a block's
    execution flags changed) and one arena per (device, stream)."""

    def __init__(self, net):
        check_record_sizes()
        self.net = net
        self.key = None
        self.tables = None      # (model, blocks, taps, keep, linear_mode, attn_mode)
        self.arenas = {}

    def _signature(self):
        """Everything the tables and the modes depend on, in one pass over the live modules: where each tensor lives now (`.to()` /
        `.cuda()` move a parameter's storage) and the execution flags of every block."""
        net = self.net
        bb = net.backbone
        n_live = len(bb.blocks) if bb.last_block is None else bb.last_block + 1
        sig = [bb.patch_embed.proj.weight.data_ptr(), bb.patch_embed.proj.bias.data_ptr(), bb.cls_token.data_ptr(),
               0 if bb.dist_token is None else bb.dist_token.data_ptr(), bb.pos_embed.data_ptr(), net.middle_feat_block_number, net.late_feat_block_number]
        for blk in bb.blocks[:n_live]:
            sig.extend(t.data_ptr() for t in block_tensors(blk))
            sig.append(block_switches(blk))
        for up in net.up.values():
            sig.extend(t.data_ptr() for t in tap_tensors(up))
        return tuple(sig)

    def ready(self):
        """The tables and modes for the module tree as it is now: (model, blocks, taps, keep, linear_mode, attn_mode).  Raises Unsupported
        (every time, with the reason) for a tree the executor does not run."""
        key = self._signature()
        if key != self.key:
            self.key, self.tables = key, None
            try:
                self.tables = emit(self.net) + modes(self.net)
            except Unsupported as err:
                self.tables = err
        if isinstance(self.tables, Unsupported):
            raise self.tables
        return self.tables

    def model_tables(self):
        return self.ready()[:4]

    def arena(self, nbytes, device):
        k = (device.index, _lib.stream())
        buf = self.arenas.get(k)
        if buf is None or buf.shape[0] < nbytes:
            if buf is not None:
                _lib.load().ftx_vit_eval_release(buf.data_ptr())      # the library's note about the arena that goes away
            buf = self.arenas[k] = torch.empty((int(nbytes),), dtype=torch.uint8, device=device)
        return buf

    def release(self):
        """Drop the arenas and the library's notes about them."""
        L = _lib.load()
        for buf in self.arenas.values():
            L.ftx_vit_eval_release(buf.data_ptr())
        self.arenas = {}

    def __del__(self):
        try:
            self.release()
        except Exception:      # interpreter shutdown: the library may be gone
            pass

    def begin(self, x):
        """Size the arena for the resampled image x (b, C, S, S) and allocate the tap outputs; returns the run whose `run(first, last)`
        issues blocks [first, last] and returns the grids of the taps among them."""
        # as ready() left them for this forward (Net2DBillinear asks it first); a direct caller gets them here
        model, blocks, taps, _, linear_mode, attn_mode = self.tables if isinstance(self.tables, tuple) else self.ready()
        x = _lib.req(x.contiguous(), torch.float32, "native image input", 4)
        b = x.shape[0]
        m = model[0]
        if tuple(x.shape[1:]) != (int(m["in_chans"]), int(m["grid"] * m["patch"]), int(m["grid"] * m["patch"])):
            raise ValueError("native image eval: the image does not match the patch grid")
        need = arena_bytes(model, len(blocks), b)
        g = int(m["grid"])
        outs = [torch.empty((b, g, g, int(t["co"])), dtype=torch.float32, device=x.device) for t in taps]
        return _Run(model, blocks, taps, linear_mode, attn_mode, x, self.arena(need, x.device), outs)


class _Run:
    def __init__(self, model, blocks, taps, linear_mode, attn_mode, x, arena, outs):
        self.model, self.blocks, self.taps, self.linear_mode, self.attn_mode = model, blocks, taps, linear_mode, attn_mode
        self.x, self.arena, self.outs = x, arena, outs

    def run(self, first, last):
        """Blocks [first, last]; returns {block index: grid (b, gh, gw, co)} of the taps the call wrote."""
        n = sum(1 for t in self.taps if int(t["block"]) <= last)
        b = self.x.shape[0]
        spf._log_launch("vit_eval", dict(b=b, first=first, last=last, linear_mode=self.linear_mode, attn_mode=self.attn_mode), lambda: eval_call(
            self.model, self.blocks, self.taps, b, self.x if first == 0 else None, None, first, last, self.linear_mode, self.attn_mode, self.outs[:n],
            self.arena))
        return {int(t["block"]): o for t, o in zip(self.taps[:n], self.outs) if first <= int(t["block"])}
