"""DeiT-base-distilled-384 trunk with per-block outputs.

Mirror of FusionTransformer/models/transformers.py:11-45,90-100.  timm is not a
dependency: the VisionTransformer structure of timm 0.4.9 (PatchEmbed, Block,
Attention, Mlp; LayerNorm eps 1e-6, exact GELU, qkv_bias=True, distilled) is
restated here with the same attribute names, so DeiT checkpoints keyed
`backbone.blocks.0.attn.qkv.weight` etc. load unchanged.

The dense contractions (patch-embed conv, qkv / proj / MLP linears) go through
torch's hipBLASLt GEMMs; softmax(QK^T/8)V runs in libftx's fused attention
kernel when `attn_impl == "ftx"` (exact fp32), `"ftx_bf16"` (bf16 operands, fp32 accumulation and softmax:
functional.attention(bf16=True)) or `"ftx_split"` (fp32-accurate on the bf16 MFMA: every operand in three bf16 pieces,
functional.attention(operands="split")), otherwise as the three explicit ops timm uses.

`SpatialTransformer` / `ScaleUpModule` (reference models/transformers.py:102-156) are at the end of the file: learned affine
resampling on libftx's affine-sampling kernels (functional.affine_sample / affine_lift)."""
from __future__ import annotations

import contextlib
import gc
from functools import partial
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ["Image2DTransformer", "image_2d_distilled_transformer", "SpatialTransformer", "ScaleUpModule"]


_ONES = {}


def _ones_row(m, like):
    key = (m, like.device, like.dtype)
    if key not in _ONES:
        _ONES[key] = torch.ones(1, m, device=like.device, dtype=like.dtype)
    return _ONES[key]


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b with the bias gradient from libftx's column-sum kernels (ftx_colsum) instead of autograd's sum_to reduction:
    that reduction kernel's result changes between the first and the later replays of a captured backward on torch 2.10 / ROCm 7
    (tools/probes/graph_block4.py), so it cannot stay in a trunk that replays as a HIP graph.  Round 1 used a (1, M) x (M, N) library
    GEMM for it (14 us per Linear at batch 4, 48 per step); the two column-sum launches take 3-6 us."""

    @staticmethod
    def forward(ctx, x, w, b, bf16=False):
        # b None: the caller adds the bias itself (Block.chain hands it to the fused add + LayerNorm that consumes this output)
        x2 = x.reshape(-1, x.shape[-1])
        ctx.in_shape, ctx.bf16 = x.shape, bool(bf16)
        if bf16:
            # BASELINE configs[4] ("bf16 forward"): operands rounded to bf16, products accumulated in fp32 by the bf16 MFMA
            # path, result and bias add in fp32; the two backward GEMMs run the same way, the bias gradient stays fp32
            x2, w = x2.to(torch.bfloat16), w.to(torch.bfloat16)
            ctx.save_for_backward(x2, w)
            y = (x2 @ w.t()).float()
            return (y.add_(b) if b is not None else y).view(*x.shape[:-1], w.shape[0])
        ctx.save_for_backward(x2, w)
        y = torch.addmm(b, x2, w.t()) if b is not None else x2 @ w.t()
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        db = None
        if ctx.needs_input_grad[2]:
            # column sums by libftx (float64, fixed order); a width that is not a multiple of 4 goes to the skinny GEMM
            if dy2.shape[1] % 4 == 0:
                from .. import functional as spf
                db = spf.colsum(dy2)
            else:
                db = (_ones_row(dy2.shape[0], dy2) @ dy2).view(-1)
        if ctx.bf16:
            dy2 = dy2.to(torch.bfloat16)
        dx = (dy2 @ w).float().view(ctx.in_shape) if ctx.needs_input_grad[0] else None
        dw = (dy2.t() @ x2).float() if ctx.needs_input_grad[1] else None
        return dx, dw, db, None


class _BatchBroadcast(torch.autograd.Function):
    """p (1, ...) -> p expanded over a batch of b; the gradient (the sum over the batch) by ftx_colsum instead of autograd's sum_to
    reduction, which does not replay reliably inside a captured backward (see _LinearFn)."""

    @staticmethod
    def forward(ctx, p, b):
        ctx.pshape = p.shape
        return p.expand(b, *p.shape[1:])

    @staticmethod
    def backward(ctx, g):
        from .. import functional as spf
        b = g.shape[0]
        g2 = g.reshape(b, -1)
        if g2.is_cuda and g2.dtype == torch.float32 and g2.shape[1] % 4 == 0:
            return spf.colsum(g2).view(ctx.pshape), None
        return g2.sum(0).view(ctx.pshape), None


def _over_batch(p, b):
    return _BatchBroadcast.apply(p, b) if p.is_cuda else p.expand(b, *p.shape[1:])


def linear_switches(lin):
    """(impl, bf16) of a trunk Linear as set_linear_impl / set_bf16 left them: the one reader of the two attributes and their defaults."""
    return getattr(lin, "ftx_linear_impl", "library"), bool(getattr(lin, "ftx_bf16", False))


# What linear_route answers.  The two own-kernel routes are spelled as the `mode` of functional.vit_linear / vit_mlp.
LIBRARY_FP32, LIBRARY_BF16, OWN_BF16, OWN_SPLIT = "library_fp32", "library_bf16", "bf16", "split"
OWN_ROUTES = (OWN_BF16, OWN_SPLIT)


def linear_route(lin):
    """Which GEMMs a trunk Linear runs on, from its two switches: "ftx_split" is the more specific request and routes to the split
    kernels whatever set_bf16 says; "ftx" routes to the bf16 kernels only with set_bf16 on; everything else is the library path, in
    bf16 or fp32."""
    impl, bf16 = linear_switches(lin)
    if impl == "ftx_split":
        return OWN_SPLIT
    if impl == "ftx" and bf16:
        return OWN_BF16
    return LIBRARY_BF16 if bf16 else LIBRARY_FP32


def block_linears(blk):
    return blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2


def block_switches(blk):
    """(attn_impl, (linear_switches of qkv, proj, fc1, fc2)): every switch of a Block, raw, as graph keys and table signatures record it."""
    return blk.attn.attn_impl, tuple(linear_switches(lin) for lin in block_linears(blk))


def _linear(x, lin, with_bias=True):
    bias = lin.bias if with_bias else None
    if lin.bias is None or not x.is_cuda:
        return F.linear(x, lin.weight, bias)
    route = linear_route(lin)
    if route in OWN_ROUTES:
        from .. import functional as spf
        return spf.vit_linear(x, lin.weight, bias, mode=route)   # the library path (fp32 for "split") for shapes the kernels do not take
    return _LinearFn.apply(x, lin.weight, bias, route == LIBRARY_BF16)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features, drop=0.0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x, with_fc2_bias=True):
        if self._fused_ftx(x):
            # vit_linear_impl "ftx" / "ftx_split": fc1 + GELU + fc2 as one node on the bf16 / three-piece split kernels (GELU in fc1's
            # epilogue, its derivative in fc2's dX)
            from .. import functional as spf
            return spf.vit_mlp(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias if with_fc2_bias else None,
                               mode=linear_route(self.fc1))
        return self.drop(_linear(self.drop(self.act(_linear(x, self.fc1))), self.fc2, with_fc2_bias))

    def _fused_ftx(self, x):
        route = linear_route(self.fc1)
        return (x.is_cuda and route in OWN_ROUTES and linear_route(self.fc2) == route
                and type(self.act) is nn.GELU and self.act.approximate == "none" and self.drop.p == 0.0
                and self.fc1.bias is not None and self.fc2.bias is not None)


# attn_impl values that run libftx's fused attention kernels, and the operand mode of functional.attention each one names; any other
# value ("torch") is the three explicit ops
ATTN_OPERANDS = {"ftx": "fp32", "ftx_bf16": "bf16", "ftx_split": "split"}


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.attn_impl = "ftx"

    def forward(self, x, with_proj_bias=True):
        B, N, C = x.shape
        qkv = _linear(x, self.qkv)
        if self.attn_impl in ATTN_OPERANDS:
            from .. import functional as spf
            x = spf.attention(qkv.view(B, N, 3, self.num_heads, C // self.num_heads), self.scale, operands=ATTN_OPERANDS[self.attn_impl])
        else:
            qkv = qkv.reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
            q, k, v = qkv[0], qkv[1], qkv[2]
            attn = (q @ k.transpose(-2, -1)) * self.scale
            attn = attn.softmax(dim=-1)
            attn = self.attn_drop(attn)
            x = (attn @ v).transpose(1, 2).reshape(B, N, C)
        return self.proj_drop(_linear(x, self.proj, with_proj_bias))


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias)
        self.drop_path = nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def forward(self, x):
        if not self._fused(x):
            x = x + self.drop_path(self.attn(self.norm1(x)))
            x = x + self.drop_path(self.mlp(self.norm2(x)))
            return x
        return _materialize(*self.chain(x, None, None))

    def _fused(self, x):
        from .. import functional as spf
        return (spf.layer_norm_supported(x) and type(self.norm1) is nn.LayerNorm and type(self.norm2) is nn.LayerNorm
                and self.norm1.elementwise_affine and self.norm2.elementwise_affine and self.norm1.bias is not None and self.norm2.bias is not None
                and self.attn.proj.bias is not None and self.mlp.fc2.bias is not None and self.attn.proj_drop.p == 0.0 and self.mlp.drop.p == 0.0
                and isinstance(self.drop_path, nn.Identity))

    def chain(self, r, p, pb):
        """The block on a residual stream held as (r, p, pb) with value r + (p + pb) (p None: just r; pb: the bias that the Linear
        which produced p did NOT add); returns it in the same form, (s2, m, fc2.bias) with the MLP output m not yet added and
        computed without its bias (`_materialize` turns the triple into one tensor, in the same rounding order).  Each LayerNorm runs fused with the add in front of it (libftx ftx_add_layernorm_*): the
        add of the previous block's MLP output with norm1, the add of the attention output with norm2 -- same arithmetic in the same
        rounding order, a third of the launches (forward: add + LayerNorm -> 1; backward: 3 LayerNorm-gradient kernels + the
        residual-gradient add + the column sums for the proj / fc2 bias gradients -> 2)."""
        from .. import functional as spf
        n1, n2 = self.norm1, self.norm2
        if p is None:
            s, h = r, spf.layer_norm(r, n1.weight, n1.bias, n1.eps)
        else:
            s, h = spf.add_layer_norm(r, p, n1.weight, n1.bias, n1.eps, y_bias=pb)
        s2, h2 = spf.add_layer_norm(s, self.attn(h, with_proj_bias=False), n2.weight, n2.bias, n2.eps, y_bias=self.attn.proj.bias)
        return s2, self.mlp(h2, with_fc2_bias=False), self.mlp.fc2.bias


class _Materialize(torch.autograd.Function):
    """r + (p + pb) with pb broadcast over the rows; the bias gradient by ftx_colsum (float64, fixed order) instead of autograd's sum_to
    reduction, which must not run inside a captured backward (see _LinearFn)."""

    @staticmethod
    def forward(ctx, r, p, pb):
        return r + (p + pb)

    @staticmethod
    def backward(ctx, g):
        gb = None
        if ctx.needs_input_grad[2]:
            g2 = g.reshape(-1, g.shape[-1])
            if g2.is_cuda and g2.dtype == torch.float32 and g2.shape[1] % 4 == 0:
                from .. import functional as spf
                gb = spf.colsum(g2)
            else:
                gb = g2.sum(0)
        return g, g, gb


def _materialize(r, p, pb):
    """r + (p + pb): the residual stream of Block.chain as one tensor (bias first, as a GEMM's bias epilogue rounds it)."""
    if p is None:
        return r
    return _Materialize.apply(r, p, pb)


class PatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patch_size = (patch_size, patch_size)
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.Identity()

    def forward(self, x):
        # Conv2d(k=16, s=16) == non-overlapping unfold + one GEMM (hipBLASLt); same arithmetic as
        # timm's self.proj(x).flatten(2).transpose(1, 2) without a convolution-library search
        B, C, H, W = x.shape
        ph, pw = self.patch_size
        gh, gw = H // ph, W // pw
        patches = x.reshape(B, C, gh, ph, gw, pw).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * ph * pw)
        w2 = self.proj.weight.view(self.proj.out_channels, -1)
        if x.is_cuda and self.proj.bias is not None and self.proj.out_channels % 4 == 0:
            return self.norm(_LinearFn.apply(patches, w2, self.proj.bias, False))    # bias gradient by ftx_colsum, not autograd's sum_to (see _LinearFn)
        return self.norm(F.linear(patches, w2, self.proj.bias))


class Image2DTransformer(nn.Module):
    def __init__(self, remove_tokens_outputs=False, img_size=384, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4.0, qkv_bias=True, distilled=True, last_block=None, **_unused):
        super().__init__()
        self.remove_tokens_outputs = remove_tokens_outputs
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens = 2 if distilled else 1
        norm_layer = partial(nn.LayerNorm, eps=1e-6)
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.dist_token = nn.Parameter(torch.zeros(1, 1, embed_dim)) if distilled else None
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + self.num_tokens, embed_dim))
        self.pos_drop = nn.Dropout(p=0.0)
        self.blocks = nn.Sequential(*[Block(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)   # kept for checkpoint compatibility; forward_blocks never applies it
        self.head = nn.Identity()           # reset_classifier(0, '') in image_models_billinear.py:44,57
        self.head_dist = nn.Identity()
        # Blocks after `last_block` never influence an output the model returns
        # (SURVEY Appendix A.12); they are skipped when it is set.
        self.last_block = last_block
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        if self.dist_token is not None:
            nn.init.trunc_normal_(self.dist_token, std=0.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.zeros_(m.bias)
                nn.init.ones_(m.weight)

    def set_bf16(self, on: bool = True):
        """bf16 operands for the qkv / proj / MLP GEMMs of every block (fp32 accumulate, fp32 everywhere else: LayerNorm,
        softmax, residual stream, attention kernel).  No counterpart in the reference, which is fp32 end to end; the parity
        bar for this mode is stated in tests/test_model_gpu.py.  The attention kernel gets bf16 operands separately:
        set_attention_impl("ftx_bf16")."""
        for blk in self.blocks:
            for lin in block_linears(blk):
                lin.ftx_bf16 = bool(on)

    def set_linear_impl(self, impl: str):
        """How the bf16 qkv / proj / fc1 / fc2 GEMMs run: "library" (torch's bf16 GEMMs, bf16 results widened to fp32, separate cast,
        bias and GELU kernels) or "ftx" (libftx's ftx_dense_* kernels: bf16 operands, fp32 accumulation and fp32 results, bias and GELU
        fused into the GEMM epilogues).  For these two, precision is still switched by set_bf16: with set_bf16(False) they change nothing.
        "ftx_split" is the fp32 model's own path: libftx's ftx_dense_*_split kernels split every fp32 operand into three bf16 pieces and
        sum six piece products in fp32 on the bf16 MFMA (fp32-class results, same fused epilogues; contract in include/ftx.h).  It is the
        more specific request, so it routes whether or not set_bf16 is on."""
        if impl not in ("library", "ftx", "ftx_split"):
            raise ValueError(f"vit_linear_impl must be 'library', 'ftx' or 'ftx_split', got {impl!r}")
        for blk in self.blocks:
            for lin in block_linears(blk):
                lin.ftx_linear_impl = impl

    def set_attention_impl(self, impl: str):
        """attn_impl of every block: "ftx" (exact fp32 MFMA, the default), "ftx_bf16", "ftx_split" (ATTN_OPERANDS) or the explicit ops."""
        for blk in self.blocks:
            blk.attn.attn_impl = impl

    def set_switches(self, kw):
        """The three switches above, set_native_train and set_native_stems from an image model's backbone_2d_kwargs (cfg.MODEL.attn_impl
        / vit_bf16 / vit_linear_impl / image_native_train / image_native_stems)."""
        self.set_attention_impl(kw.get("attn_impl", "ftx"))
        if kw.get("vit_bf16", False):
            self.set_bf16(True)   # BASELINE configs[4] "bf16 forward"; default is fp32 like the reference
        self.set_linear_impl(kw.get("vit_linear_impl", "library"))
        self.set_native_train(bool(kw.get("image_native_train", False)))      # cfg.MODEL.image_native_train
        self.set_native_stems(bool(kw.get("image_native_stems", False)))      # cfg.MODEL.image_native_stems

    # ---- native training executor of the trunk -------------------------------------------------------------
    image_native_train = False

    def set_native_train(self, on=True):
        """Opt-in native executor for the training passes of the trunk (include/ftx.h: ftx_vit_train_fwd / ftx_vit_train_bwd).  With it
        on, a forward in training mode with gradients enabled, on float32 CUDA tensors and outside a stream capture, runs `_embed` as
        before and then every trunk segment -- the segments of `_segment_ends()` when `graph_taps` is set, every live block otherwise:
        those of the eager path -- as one autograd node whose forward and backward are one library call each
        (native_image_train._VitSegment), issuing the kernels of Block.chain in its order: outputs, gradients and parameters after the
        step are bit-identical to the switch being off.  It needs no capture, no static buffers and no per-shape state, and it runs
        after an eager pass.  It engages only when every live block passes Block._fused, runs the linears the library owns
        (vit_linear_impl "ftx_split", or "ftx" with set_bf16) and one attention impl of "ftx", "ftx_bf16", "ftx_split", and every
        parameter of the live blocks requires a gradient; anything else takes the existing path exactly as with the switch off, and
        native_train_reason() says why.  Asked before the HIP graphs; like an eager pass it ends new captures on this trunk."""
        self.image_native_train = bool(on)
        if not on:
            self.__dict__["_native_tr"] = None
            self.__dict__["_native_tr_reason"] = "the switch is off"
        return self

    def native_train_reason(self):
        """Why the last forward_blocks did not run the native training executor; None when it did."""
        return self.__dict__.get("_native_tr_reason", "the switch is off")

    def _native_trainer(self, x):
        """The training executor when this forward is one it runs (see set_native_train), else None (and the reason is kept)."""
        why = None
        if not self.image_native_train:
            why = "the switch is off"
        elif not self.training:
            why = "eval mode"
        elif not torch.is_grad_enabled():
            why = "gradients are disabled"
        elif not x.is_cuda or x.dtype != torch.float32:
            why = "the input is not a float32 tensor on the GPU"
        elif torch.cuda.is_current_stream_capturing():
            why = "the stream is being captured"
        else:
            live = [b for i, b in enumerate(self.blocks) if self.last_block is None or i <= self.last_block]
            probe = x.new_empty((0, self.embed_dim))      # what Block._fused asks of the tokens: device, dtype and width
            if not all(b._fused(probe) for b in live):
                why = "a live block does not run the fused chain (Block._fused)"
            elif not all(p.requires_grad for b in live for p in b.parameters()):
                why = "a parameter of a live block is frozen (requires_grad is off)"
            else:
                from .. import native_image_train as nit
                try:
                    ex = self.__dict__.get("_native_tr")
                    if ex is None:
                        ex = self.__dict__["_native_tr"] = nit.NativeImageTrain(self)
                    ex.ready()      # one pass over the live blocks; the table and the modes are cached behind it
                except nit.Unsupported as err:
                    why = str(err)
        self.__dict__["_native_tr_reason"] = why
        return self.__dict__["_native_tr"] if why is None else None

    def _forward_native_train(self, ex, x, on_block, full_tokens=False):
        """forward_blocks through the training executor: `_embed` here, then one node per segment.  As on the graphed path only segment
        ends exist as tensors: the taps' outputs with `graph_taps` set, every block's without."""
        # as after an eager pass (forward_blocks): a capture attempted behind a backward through these parameters aborts the process
        self._capture_off("the native training executor ran through the trunk before the capture")
        x = self._embed(x)
        n_live = len(self.blocks) if self.last_block is None else self.last_block + 1
        taps = set(int(t) for t in self.graph_taps) if self.graph_taps else None
        outputs, first = dict(), 0
        for e in (self._segment_ends() if self.graph_taps else range(n_live)):
            x = ex.segment(x, first, e)
            first = e + 1
            if taps is None or e in taps:
                outputs[str(e)] = self._tap_view(x, full_tokens)
                if on_block is not None:
                    on_block(e, outputs[str(e)])
        return outputs

    # ---- patch embedding and tap stems on the library's kernels in training ---------------------------------
    image_native_stems = False

    def set_native_stems(self, on=True):
        """Opt-in library path for the two places where the image branch still leaves the library in training (cfg.MODEL.
        image_native_stems): the patch embedding (`_embed`: unfold copy, GEMM, + pos, the cls / dist rows and their gradients become
        functional.vit_patch_embed, one node on ftx_vit_patch_embed_* / ftx_vit_patch_embed_bwd_*) and, in Net2DBillinear, the tap stems
        (functional.vit_tap_stem).  It engages in training mode with gradients enabled on float32 CUDA tensors, exactly where the native
        image executors engage: every live block runs the linears the library owns (vit_linear_impl "ftx_split", or "ftx" with
        set_bf16), whose mode the stems take.  Anything else takes the existing path exactly as with the switch off, and
        native_stems_reason() says why.  Independent of set_native_train and of the HIP graphs (the nodes are capturable)."""
        self.image_native_stems = bool(on)
        if not on:
            self.__dict__["_native_stems_reason"] = "the switch is off"
        return self

    def native_stems_reason(self):
        """Why the last embedding did not run on the library's training forms; None when it did."""
        return self.__dict__.get("_native_stems_reason", "the switch is off")

    def native_stems_mode(self, x):
        """The mode ("split" | "bf16") of functional.vit_patch_embed / vit_tap_stem when a forward on the image x is one the native
        stems run (see set_native_stems), else None (and the reason is kept)."""
        why, mode = None, None
        if not self.image_native_stems:
            why = "the switch is off"
        elif not self.training:
            why = "eval mode"
        elif not torch.is_grad_enabled():
            why = "gradients are disabled"
        elif not x.is_cuda or x.dtype != torch.float32:
            why = "the input is not a float32 tensor on the GPU"
        else:
            live = [b for i, b in enumerate(self.blocks) if self.last_block is None or i <= self.last_block]
            routes = {linear_route(lin) for b in live for lin in block_linears(b)}
            pe = self.patch_embed
            if len(routes) != 1 or next(iter(routes)) not in OWN_ROUTES:
                impl, bf16 = linear_switches(live[0].attn.qkv) if live else ("library", False)
                why = ("vit_linear_impl is %r%s: the stems take the mode of the trunk's own linears ('ftx_split', or 'ftx' with set_bf16)"
                       % (impl, "" if impl != "ftx" or bf16 else " without set_bf16"))
            elif pe.proj.bias is None or not isinstance(pe.norm, nn.Identity) or self.pos_drop.p != 0.0:
                why = "the patch embedding has no bias, a norm or a dropout"
            else:
                from .. import functional as spf
                if not spf.vit_patch_embed_supported(x, pe.proj.weight):
                    why = "the kernels do not take this embedding (patch % 4, c patch patch % 64, dim % 64, whole patches)"
                else:
                    mode = next(iter(routes))
        self.__dict__["_native_stems_reason"] = why
        return mode

    def _tap_view(self, t, full_tokens=False):
        """A block's output as the caller gets it: without the cls / dist rows when `remove_tokens_outputs` is set and the caller
        did not ask for the whole tokens."""
        return t[:, self.num_tokens:, :] if self.remove_tokens_outputs and not full_tokens else t

    def _embed(self, x):
        mode = self.native_stems_mode(x)
        if mode is not None:
            from .. import functional as spf
            pe = self.patch_embed
            return self.pos_drop(spf.vit_patch_embed(x, pe.proj.weight, pe.proj.bias, self.cls_token, self.dist_token, self.pos_embed, mode=mode))
        x = self.patch_embed(x)
        b = x.shape[0]
        cls_token = _over_batch(self.cls_token, b)
        if self.dist_token is None:
            x = torch.cat((cls_token, x), dim=1)
        else:
            x = torch.cat((cls_token, _over_batch(self.dist_token, b), x), dim=1)
        return self.pos_drop(x + _over_batch(self.pos_embed, b))

    def forward_blocks(self, x: torch.Tensor, on_block=None, full_tokens=False) -> Dict[str, torch.Tensor]:
        """reference models/transformers.py:16-45: every block's output, cls/dist tokens stripped.
        `on_block(i, tokens)` is called as soon as block i's output exists (used to lift the tapped
        block's features while the remaining blocks are still being issued).
        `full_tokens`: the outputs keep their leading cls / dist rows whatever `remove_tokens_outputs` says; a caller that skips them
        by addressing (functional.vit_tap_stem under set_native_stems) asks for that.

        With `graph_taps` set (training on the GPU) the trunk runs as one HIP graph per tapped segment --
        forward and backward: the shapes are static, and ~500 kernel launches per step become 2 x 2 graph
        launches.  Only the tapped blocks' outputs are returned then (the model reads no others)."""
        trainer = self._native_trainer(x)
        if trainer is not None:
            return self._forward_native_train(trainer, x, on_block, full_tokens)
        graphed = self._graphed_segments(x)
        if graphed is not None:
            outputs = dict()
            for last, seg, is_tap in graphed:
                x = seg(x)
                if is_tap:
                    outputs[str(last)] = self._tap_view(x, full_tokens)
                    if on_block is not None:
                        on_block(last, outputs[str(last)])
            return outputs
        infer = self._inference_graph(x)
        if infer is not None:
            # validate()'s forward (data/utils/validate.py:59): the whole live trunk as ONE forward-only HIP graph; the tapped outputs
            # are copies, so a later replay does not change tensors the caller still holds
            outputs = dict()
            for i, t in infer(x):
                outputs[str(i)] = self._tap_view(t, full_tokens)
                if on_block is not None:
                    on_block(i, outputs[str(i)])
            return outputs
        if x.is_cuda and self.training and torch.is_grad_enabled():
            # This pass and its backward run eagerly.  A capture attempted AFTER an eager backward through these parameters
            # aborts the process inside hipStreamEndCapture on torch 2.10 / ROCm 7 (tools/probes/graph_recapture.py) -- an abort,
            # not an exception -- so from here on no NEW capture is attempted (already captured shapes keep replaying).
            self._capture_off("an eager training pass ran through the trunk before the capture")
        outputs = dict()

        def emit(i, t):
            outputs[str(i)] = self._tap_view(t, full_tokens)
            if on_block is not None:
                on_block(i, outputs[str(i)])

        self._forward_eager(x, emit)
        return outputs

    def _forward_eager(self, x, emit, want=None):
        """The live blocks, eagerly; emit(i, tokens) for every block i (want=None: what the reference's forward_blocks returns) or only
        for the blocks in `want`.

        Same residual-stream form as the captured segments (_TrunkSegment): inside a segment the stream stays (r, p, pb) from block to
        block, at a segment end it becomes one tensor -- so the eager trunk and the graphed trunk run the SAME kernels in the same order
        and agree to the last bit in every gradient.  A block's output in between is materialised for the caller only."""
        x = self._embed(x)
        live = [b for i, b in enumerate(self.blocks) if self.last_block is None or i <= self.last_block]
        ends = set(self._segment_ends()) if self.graph_taps else None      # no taps known: every block ends a segment
        chained = x.is_cuda and ends is not None and all(b._fused(x) for b in live)
        r, p, pb = x, None, None
        for i, block in enumerate(live):
            need = want is None or i in want
            if chained:
                r, p, pb = block.chain(r, p, pb)
                if i in ends:
                    x = _materialize(r, p, pb)
                    r, p, pb = x, None, None
                elif need:
                    x = _materialize(r, p, pb)
            else:
                x = block(x)
            if need:
                emit(i, x)

    # ---- HIP-graph execution of the trunk ------------------------------------------------------------------
    graph_taps = None   # sorted block indices whose outputs the caller uses; None: eager execution
    graph_segment_blocks = 3   # blocks per captured segment (a tap always ends one)

    def _graph_key(self, x):
        """Everything a captured graph bakes in: input shape / dtype / requires_grad, the tap set and segment length, the
        per-block execution switches and the parameters' requires_grad pattern.  Changing any of them selects another graph."""
        grads = tuple(p.requires_grad for p in self.parameters())
        return (tuple(x.shape), x.dtype, bool(x.requires_grad), tuple(self.graph_taps), self.last_block, self.graph_segment_blocks,
                tuple(block_switches(blk) for blk in self.blocks), grads, torch.cuda.current_device(), bool(self.image_native_stems))

    def _graphed_segments(self, x):
        if not self.graph_taps or not self.use_graphs or not x.is_cuda or not self.training or not torch.is_grad_enabled():
            return None
        cache = self.__dict__.setdefault("_graph_cache", {})
        key = self._graph_key(x)
        if key not in cache:
            if self.__dict__.get("_graph_capture_off", False):
                # an eager training pass or a refused capture came before: never capture again (see forward_blocks); say so ONCE
                if not self.__dict__.get("_graph_off_reported", False):
                    import sys
                    self.__dict__["_graph_off_reported"] = True
                    print("[fusiontransformer_amd] ViT trunk runs eagerly for input %s: HIP-graph capture is off (%s)"
                          % (tuple(x.shape), self.__dict__.get("_graph_off_reason", "unknown")), file=sys.stderr, flush=True)
                return None
            try:
                cache[key] = self._capture_segments(x)
            except Exception as err:   # capture refused (another thread touched the device, unsupported op, ...): run eagerly
                import sys
                print("[fusiontransformer_amd] HIP-graph capture of the ViT trunk failed (%s: %s); running it eagerly from now on" % (type(err).__name__, err),
                      file=sys.stderr, flush=True)
                cache[key] = None
                self._capture_off("capture refused: %s: %s" % (type(err).__name__, err))
        return cache[key]

    # ---- forward-only graph for evaluation -----------------------------------------------------------------------------------
    eval_graphs = True

    def _infer_key(self, x):
        """The forward-only graph's counterpart of _graph_key (no gradients, so no requires_grad patterns)."""
        return (tuple(x.shape), x.dtype, tuple(self.graph_taps), self.last_block, tuple(block_switches(blk) for blk in self.blocks),
                torch.cuda.current_device())

    def _inference_graph(self, x):
        """Replay function of the forward-only HIP graph for this input shape, or None (not on the GPU, gradients enabled, training
        mode, taps unknown, or the capture was refused).  No autograd node is created under no_grad, so the restriction of the
        training capture (never after an eager backward, see forward_blocks) does not apply."""
        if (not self.eval_graphs or not self.graph_taps or not self.use_graphs or not x.is_cuda or self.training or torch.is_grad_enabled()
                or torch.cuda.is_current_stream_capturing()):
            return None
        cache = self.__dict__.setdefault("_infer_cache", {})
        key = self._infer_key(x)
        if key not in cache:
            try:
                cache[key] = self._capture_inference(x)
            except Exception as err:     # refused: run eagerly from now on for this shape
                import sys
                print("[fusiontransformer_amd] forward-only HIP-graph capture of the ViT trunk failed (%s: %s); evaluation runs it eagerly" % (type(err).__name__, err),
                      file=sys.stderr, flush=True)
                cache[key] = None
        return cache[key]

    def _capture_inference(self, x):
        taps = sorted(int(t) for t in self.graph_taps)
        static_in = x.detach().clone()

        def run(inp):
            got = {}
            self._forward_eager(inp, lambda i, t: got.__setitem__(i, t), want=set(taps))
            return [got[t] for t in taps]

        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                run(static_in)                                  # warm-up: lazy initialisation, TunableOp selections, scratch growth
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with _no_gc(), torch.no_grad(), torch.cuda.graph(graph):
            static_out = run(static_in)

        def replay(inp):
            static_in.copy_(inp)
            graph.replay()
            return [(t, o.clone()) for t, o in zip(taps, static_out)]

        return replay

    def _capture_off(self, reason):
        if not self.__dict__.get("_graph_capture_off", False):
            self.__dict__["_graph_capture_off"] = True
            self.__dict__["_graph_off_reason"] = str(reason)

    def graph_state(self):
        """"on" (every shape seen so far replays as HIP graphs), "off:<reason>" (capture was switched off: later shapes run eagerly,
        at a cost in speed only), "eager" (graph_taps not set), "idle" (nothing captured yet)."""
        if not self.graph_taps or not self.use_graphs:
            return "eager"
        if self.__dict__.get("_graph_capture_off", False):
            return "off:" + self.__dict__.get("_graph_off_reason", "unknown")
        cache = self.__dict__.get("_graph_cache") or {}
        if not cache:
            return "idle"
        return "on" if all(v is not None for v in cache.values()) else "off:a capture fell back to eager execution"

    use_graphs = True    # False: same segment structure, executed eagerly (the twin of bench.py's selfcheck and of the bit-identity tests)

    def _segment_ends(self):
        """Last block of every trunk segment: every tap, and at most `graph_segment_blocks` blocks per segment -- the gradients of a
        segment become available together when its backward graph has run, so shorter segments keep the data-parallel bucket
        all-reduces (dist.GradReducer) overlapped with the rest of the backward."""
        ends, first = [], 0
        for t in sorted(int(t) for t in self.graph_taps):
            while t - first + 1 > self.graph_segment_blocks:
                ends.append(first + self.graph_segment_blocks - 1)
                first = ends[-1] + 1
            ends.append(t)
            first = t + 1
        return ends

    def _capture_segments(self, x):
        taps = sorted(int(t) for t in self.graph_taps)
        ends = self._segment_ends()
        segments, first = [], 0
        for e in ends:
            segments.append(_TrunkSegment(self, first, e, embed=(first == 0)))
            first = e + 1
        # sample inputs with the live requires_grad pattern (the resampled image carries the gradient of sample_down)
        samples = [(x.detach().clone().requires_grad_(x.requires_grad),)]
        with torch.no_grad():
            h = segments[0](samples[0][0])
            for seg in segments[1:]:
                samples.append((h.detach().clone().requires_grad_(True),))
                h = seg(h)
        with _no_gc():
            graphed = torch.cuda.make_graphed_callables(tuple(segments), tuple(samples), num_warmup_iters=3)
        taps_set = set(taps)
        return [(e, g, e in taps_set) for e, g in zip(ends, graphed)]


@contextlib.contextmanager
def _no_gc():
    """Python's cyclic garbage collector off while a trunk graph is captured: a collection that starts inside the capture can finalise
    an earlier object that releases a GPU resource, which the runtime refuses during capture (an abort, not an exception)."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class _TrunkSegment(nn.Module):
    """Blocks first..last of a trunk (plus the embedding for the first segment) as one capturable callable.  It shares
    the trunk's modules and parameters; it is never registered in the model, so state_dict keys do not change."""

    def __init__(self, trunk, first, last, embed):
        super().__init__()
        self.embed = embed
        if embed:
            object.__setattr__(self, "_trunk", trunk)
            self.patch_embed, self.cls_token, self.dist_token, self.pos_embed = trunk.patch_embed, trunk.cls_token, trunk.dist_token, trunk.pos_embed
        self.blocks = nn.ModuleList([trunk.blocks[i] for i in range(first, last + 1)])

    def forward(self, x):
        if self.embed:
            x = self._trunk._embed(x)
        if not all(block._fused(x) for block in self.blocks):
            for block in self.blocks:
                x = block(x)
            return x
        r, p, pb = x, None, None    # residual stream as (r, p, pb): the add of a block's MLP output (and of fc2's bias) runs inside the next block's norm1 kernel
        for block in self.blocks:
            r, p, pb = block.chain(r, p, pb)
        return _materialize(r, p, pb)


def image_2d_distilled_transformer(pretrained=False, **kwargs):
    """reference models/transformers.py:90-100 (DeiT-base distilled, patch 16, 384x384).

    `pretrained=True` would fetch weights by name; there is no network here, so it is refused."""
    if pretrained:
        raise RuntimeError("pretrained DeiT weights cannot be fetched offline; pass IMAGE_PRETRAINED_PATH or use random init")
    model_kwargs = dict(patch_size=16, embed_dim=768, depth=12, num_heads=12, img_size=384, distilled=True)
    model_kwargs.update(kwargs)
    return Image2DTransformer(**model_kwargs)


class SpatialTransformer(nn.Module):
    """reference models/transformers.py:102-135, same attribute names / state_dict keys and the same identity initialisation.

    The localisation net (Conv 7x7 -> MaxPool -> ReLU -> Conv 5x5 -> MaxPool -> ReLU -> global average -> two Linears) runs on torch's
    own ops by default, its convolutional part on own fused kernels after set_loc_impl("ftx"); the resampling F.grid_sample(x, F.affine_grid(theta, ...)) runs on libftx without the grid: `forward` is the dense form
    (every pixel of the target; differentiable in theta only), `lift` the point form (only the pixels the points pick; differentiable
    in x and theta)."""

    def __init__(self, in_channels):
        super().__init__()
        self.localization = nn.Sequential(
            nn.Conv2d(in_channels, 8, kernel_size=7),
            nn.MaxPool2d(2, stride=2),
            nn.ReLU(True),
            nn.Conv2d(8, 10 * 3 * 3, kernel_size=5),
            nn.MaxPool2d(2, stride=2),
            nn.ReLU(True),
            nn.AdaptiveAvgPool2d(1))
        self.fc_loc = nn.Sequential(
            nn.Linear(10 * 3 * 3, 32),
            nn.ReLU(True),
            nn.Linear(32, 3 * 2))
        self.fc_loc[2].weight.data.zero_()
        self.fc_loc[2].bias.data.copy_(torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.float))

    LOC_IMPLS = ("library", "ftx")

    def set_loc_impl(self, impl: str):
        """"library": the localisation net's convolutions and pools are torch's.  "ftx": on CUDA tensors its convolutional part runs as
        two fused conv + pool + ReLU layers of csrc/ftx_stn_loc.hip (functional.loc_conv_pool_relu), the second one straight to the
        spatial mean.  The parameters stay in the nn.Conv2d modules either way; `fc_loc` is untouched."""
        if impl not in self.LOC_IMPLS:
            raise ValueError(f"stn_loc_impl must be one of {self.LOC_IMPLS}, got {impl!r}")
        self.loc_impl = impl
        return self

    def theta(self, x):
        """The (B, 2, 3) affine matrices the localisation net reads off x."""
        if getattr(self, "loc_impl", "library") == "ftx" and x.is_cuda:
            from .. import functional as spf
            c1, c2 = self.localization[0], self.localization[3]
            xs = spf.loc_conv_pool_relu(x, c1.weight, c1.bias)
            xs = spf.loc_conv_pool_relu(xs, c2.weight, c2.bias, mean=True)
            return self.fc_loc(xs).view(-1, 2, 3)
        # localization[6] is AdaptiveAvgPool2d(1): the plain mean is the same number, and its backward is a broadcast, not the
        # adaptive pool's scatter
        xs = self.localization[:6](x).mean((2, 3))
        return self.fc_loc(xs).view(-1, 2, 3)

    def forward(self, x, output_shape):
        theta = self.theta(x)
        size = tuple(int(v) for v in output_shape[-2:])
        if not x.is_cuda:   # host-side checks of the module tree only; the product path is the kernel
            grid = F.affine_grid(theta, (x.shape[0], x.shape[1]) + size, align_corners=False)
            return F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        from .. import functional as spf
        return spf.affine_sample(x, theta.contiguous(), size)

    def lift(self, x, img_idx, point_batch, H, W):
        """Rows (N, C) of forward(x, (C, H, W)) at (point_batch, :, row, col) without forming the (H, W) map."""
        from .. import functional as spf
        return spf.affine_lift(x, self.theta(x).contiguous(), img_idx, point_batch, H, W)


class ScaleUpModule(nn.Module):
    """reference models/transformers.py:137-156: ConvTranspose2d(kernel = stride) then a SpatialTransformer to the output size.

    `forward(x, output_shape)` keeps the reference signature and returns the dense map.  The reference then keeps ~20 k pixels of that
    96 x 370 x 1226 map (174 MB per frame, written in the forward and again in the backward); `lift` is what the model calls instead: the
    up-convolved map exists once (the localisation net reads it), the resampled map never."""

    def __init__(self, input_features: int, output_features: int, kernel_size: int, stride: int):
        super().__init__()
        self.up_conv = nn.ConvTranspose2d(input_features, output_features, kernel_size=(kernel_size, kernel_size), stride=(stride, stride))
        self.up_stn = SpatialTransformer(in_channels=output_features)

    def up(self, x):
        """up_conv(x) as NCHW.  kernel == stride: the output patches do not overlap, so it is one GEMM over the input pixels plus a
        permute (the mirror image of PatchEmbed.forward), without a convolution-library search."""
        conv = self.up_conv
        k = conv.kernel_size
        if (k != conv.stride or conv.padding != (0, 0) or conv.output_padding != (0, 0) or conv.dilation != (1, 1) or conv.groups != 1):
            return conv(x)
        B, C, gh, gw = x.shape
        co = conv.out_channels
        rows = x.permute(0, 2, 3, 1).reshape(B * gh * gw, C)
        y = rows @ conv.weight.view(C, co * k[0] * k[1])
        y = y.view(B, gh, gw, co, k[0], k[1]).permute(0, 3, 1, 4, 2, 5).reshape(B, co, gh * k[0], gw * k[1])
        return y + conv.bias.view(1, -1, 1, 1) if conv.bias is not None else y

    def forward(self, x: torch.Tensor, output_shape: tuple) -> torch.Tensor:
        """The dense map, reference signature.  On the GPU the dense kernel gives its source no gradient and refuses one that needs it:
        call this under torch.no_grad(); training goes through `lift`."""
        return self.up_stn(self.up(x), output_shape)

    def lift(self, x, img_idx, point_batch, H, W):
        return self.up_stn.lift(self.up(x), img_idx, point_batch, H, W)
