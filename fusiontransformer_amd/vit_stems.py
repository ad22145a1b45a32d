"""The autograd nodes of the ViT's patch embedding and tap stems in training, over the library's training forms (include/ftx.h:
ftx_vit_patch_embed_*, ftx_vit_patch_embed_bwd_*, ftx_vit_tap_stem_train_fwd_*, ftx_vit_tap_stem_bwd_*).  The public entries are
functional.vit_patch_embed and functional.vit_tap_stem; the nodes follow the contract of functional.py's own: operands checked (ValueError)
before anything is launched, what the backward reads goes through save_for_backward, every gradient subset returns the bits of the
all-on run (tests/test_vit_stems_train_gpu.py)."""
import torch

from . import _lib
from ._lib import check, ptr, req, stream
from .functional import F32, _channel_operands, _empty, _log_launch, _scratch, _ws_bytes


def vit_patch_embed_supported(img, weight):
    """True when ftx_vit_patch_embed_* and its backward take this embedding: fp32 CUDA tensors, a square patch that is a multiple of 4,
    c patch patch and the width multiples of 64, whole patches."""
    if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == F32 and img.dim() == 4 and weight.is_cuda and weight.dtype == F32
            and weight.dim() == 4):
        return False
    dim, c, p, pw = weight.shape
    return (p == pw and p % 4 == 0 and img.shape[1] == c and (c * p * p) % 64 == 0 and dim % 64 == 0 and img.shape[2] % p == 0
            and img.shape[3] % p == 0 and img.shape[0] >= 1)


class _VitPatchEmbed(torch.autograd.Function):
    """tokens (b, t0 + g, dim) from img (b, c, h, w): ftx_vit_patch_embed_<mode> forward (the unfold is never written; + pos and the cls /
    dist rows in the same call), ftx_vit_patch_embed_bwd_<mode> backward: the weight gradient on the unfold addressing, d pos as the
    ordered sum over the frames, d bias / d cls / d dist from it, and the image gradient through the fold only when img asks."""

    @staticmethod
    def forward(ctx, img, w, bias, cls, dist, pos, mode):
        L = _lib.load()
        img = req(img.contiguous(), F32, "vit_patch_embed img", 4)
        w = req(w.contiguous(), F32, "vit_patch_embed weight", 4)
        b, c, h, wd = img.shape
        dim, wc, p, pw = w.shape
        if wc != c or p != pw:
            raise ValueError(f"vit_patch_embed: weight {tuple(w.shape)} does not fit an image of {c} channels with a square patch")
        if p % 4 or h % p or wd % p or (c * p * p) % 64 or dim % 64 or b < 1:
            raise ValueError(f"vit_patch_embed: the kernels take patch % 4 == 0, whole patches, c patch patch % 64 == 0, dim % 64 == 0 and "
                             f"b >= 1 (img {tuple(img.shape)}, weight {tuple(w.shape)})")
        t0 = 1 if dist is None else 2
        g = (h // p) * (wd // p)
        _channel_operands(img, dim, "vit_patch_embed", bias=bias)
        heads = dict(cls=cls) if dist is None else dict(cls=cls, dist=dist)
        shapes = {k: v.shape for k, v in heads.items()}
        for k, v in heads.items():
            if not isinstance(v, torch.Tensor) or v.numel() != dim:
                raise ValueError(f"vit_patch_embed {k}: expected {dim} elements")
        cls2 = req(cls.contiguous().view(dim), F32, "vit_patch_embed cls", 1)
        dist2 = None if dist is None else req(dist.contiguous().view(dim), F32, "vit_patch_embed dist", 1)
        if not isinstance(pos, torch.Tensor) or pos.numel() != (t0 + g) * dim:
            raise ValueError(f"vit_patch_embed pos: expected {(t0 + g) * dim} elements ({t0} + {g} rows of {dim})")
        pos2 = req(pos.contiguous().view(t0 + g, dim), F32, "vit_patch_embed pos", 2)
        for t, name in ((w, "weight"), (cls2, "cls"), (dist2, "dist"), (pos2, "pos")):
            if t is not None and t.device != img.device:
                raise ValueError(f"vit_patch_embed {name}: lives on another device than the image")
        tokens = _empty((b, t0 + g, dim), F32, img)
        fn = "ftx_vit_patch_embed_" + mode
        _log_launch("vit_patch_embed_" + mode, dict(b=b, g=g, k=c * p * p, dim=dim), lambda: check(getattr(L, fn)(
            ptr(img), ptr(w), ptr(bias), ptr(cls2), ptr(dist2), ptr(pos2), b, c, h, wd, p, dim, t0, ptr(tokens), stream()), fn))
        ctx.save_for_backward(img, w)
        ctx.mode, ctx.t0, ctx.shapes, ctx.pos_shape = mode, t0, shapes, pos.shape
        return tokens

    @staticmethod
    def backward(ctx, dtokens):
        L = _lib.load()
        img, w = ctx.saved_tensors
        mode, t0 = ctx.mode, ctx.t0
        b, c, h, wd = img.shape
        dim, _, p, _ = w.shape
        g = (h // p) * (wd // p)
        dtokens = req(dtokens.contiguous(), F32, "vit_patch_embed grad", 3)
        if tuple(dtokens.shape) != (b, t0 + g, dim):
            raise ValueError(f"vit_patch_embed grad: expected {(b, t0 + g, dim)}, got {tuple(dtokens.shape)}")
        dw = torch.empty_like(w)
        dbias, dcls = _empty((dim,), F32, img), _empty((dim,), F32, img)
        ddist = _empty((dim,), F32, img) if t0 == 2 else None
        dpos = _empty((t0 + g, dim), F32, img)
        dimg = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        ws_bytes = _ws_bytes(f"ftx_vit_patch_embed_bwd_{mode}_workspace_bytes", b, c, h, wd, p, dim)
        ws = _scratch(ws_bytes, img)
        fn = "ftx_vit_patch_embed_bwd_" + mode
        _log_launch("vit_patch_embed_bwd_" + mode, dict(b=b, g=g, k=c * p * p, dim=dim, dimg=dimg is not None), lambda: check(getattr(L, fn)(
            ptr(dtokens), ptr(img), ptr(w), b, c, h, wd, p, dim, t0, ptr(dw), ptr(dbias), ptr(dcls), ptr(ddist), ptr(dpos), ptr(dimg), ptr(ws),
            ws_bytes, stream()), fn))
        need = ctx.needs_input_grad
        return (dimg, dw if need[1] else None, dbias if need[2] else None, dcls.view(ctx.shapes["cls"]) if need[3] else None,
                ddist.view(ctx.shapes["dist"]) if t0 == 2 and need[4] else None, dpos.view(ctx.pos_shape) if need[5] else None, None)


class _VitTapStem(torch.autograd.Function):
    """rows (b g, co) = ReLU(tokens[:, t0:] W^T + bias) on ftx_vit_tap_stem_train_fwd_<mode>; backward on ftx_vit_tap_stem_bwd_<mode>
    from the saved rows (the ReLU's mask), the tokens and W."""

    @staticmethod
    def forward(ctx, tokens, w, bias, t0, mode):
        L = _lib.load()
        tokens = req(tokens.contiguous(), F32, "vit_tap_stem tokens", 3)
        b, tg, dim = tokens.shape
        t0 = int(t0)
        g = tg - t0
        if w.dim() == 4 and w.shape[2:] == (1, 1):
            w2 = w.reshape(w.shape[0], w.shape[1])
        else:
            w2 = w
        w2 = req(w2.contiguous(), F32, "vit_tap_stem weight", 2)
        co = w2.shape[0]
        if t0 not in (0, 1, 2) or g < 1 or b < 1 or w2.shape[1] != dim or dim % 64 or co % 4 or w2.device != tokens.device:
            raise ValueError(f"vit_tap_stem: the kernels take t0 in (0, 1, 2), at least one row behind it, a weight (co, {dim}) on the tokens' "
                             f"device, dim % 64 == 0 and co % 4 == 0 (tokens {tuple(tokens.shape)}, t0 {t0}, weight {tuple(w.shape)})")
        _channel_operands(tokens, co, "vit_tap_stem", bias=bias)
        rows = _empty((b * g, co), F32, tokens)
        fn = "ftx_vit_tap_stem_train_fwd_" + mode
        _log_launch("vit_tap_stem_fwd_" + mode, dict(b=b, g=g, dim=dim, co=co), lambda: check(getattr(L, fn)(
            ptr(tokens), ptr(w2), ptr(bias), b, g, t0, dim, co, ptr(rows), stream()), fn))
        ctx.save_for_backward(tokens, w2, rows)
        ctx.t0, ctx.mode, ctx.w_shape = t0, mode, w.shape
        return rows

    @staticmethod
    def backward(ctx, drows):
        L = _lib.load()
        tokens, w2, rows = ctx.saved_tensors
        mode, t0 = ctx.mode, ctx.t0
        b, tg, dim = tokens.shape
        g, co = tg - t0, w2.shape[0]
        drows = req(drows.contiguous(), F32, "vit_tap_stem grad", 2)
        if tuple(drows.shape) != (b * g, co):
            raise ValueError(f"vit_tap_stem grad: expected {(b * g, co)}, got {tuple(drows.shape)}")
        dw, dbias, dtokens = torch.empty_like(w2), _empty((co,), F32, tokens), torch.empty_like(tokens)
        ws_bytes = _ws_bytes(f"ftx_vit_tap_stem_bwd_{mode}_workspace_bytes", b, g, dim, co)
        ws = _scratch(ws_bytes, tokens)
        fn = "ftx_vit_tap_stem_bwd_" + mode
        _log_launch("vit_tap_stem_bwd_" + mode, dict(b=b, g=g, dim=dim, co=co), lambda: check(getattr(L, fn)(
            ptr(drows), ptr(rows), ptr(tokens), ptr(w2), b, g, t0, dim, co, ptr(dw), ptr(dbias), ptr(dtokens), ptr(ws), ws_bytes, stream()), fn))
        need = ctx.needs_input_grad
        return dtokens if need[0] else None, dw.view(ctx.w_shape) if need[1] else None, dbias if need[2] else None, None, None
