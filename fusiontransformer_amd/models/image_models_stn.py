"""Image branch with learned affine resampling + 2D->3D lift.

Mirror of FusionTransformer/models/image_models_stn.py:7-128 (`Net2DSeg`), same attribute names / state_dict keys: a
`SpatialTransformer` brings the picture to the ViT's 384x384 (`stn_down`), a `ScaleUpModule` per tapped block brings the
24x24 token map back to the picture (`up`).

What changes on MI355X: the reference resamples each tapped block's 96x384x384 up-convolved map to 96x370x1226 (174 MB fp32
per frame, written in the forward and again in the backward) and then picks ~20k pixels out of it.  Here `ScaleUpModule.lift`
samples the 384x384 map at those pixels directly (functional.affine_lift): the resampled map never exists.

The trunk runs eagerly in this model: its input carries the gradient of `stn_down`'s theta, a requires_grad pattern the HIP-graph
capture of the trunk has not been exercised with.  `cfg.MODEL.image_native_train` (`set_native_train`) is the other way to take the
trunk's per-op launches off the Python side: every block then runs as one autograd node of the native training executor
(Image2DTransformer.set_native_train), which delivers the input's gradient to `stn_down` and is bit-identical to the eager trunk;
it needs vit_linear_impl "ftx_split" (or "ftx" with vit_bf16).  Time of this model: not measured."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict

import torch
import torch.nn as nn

from .. import functional as spf
from .image_models_billinear import pack_img_indices
from .transformers import ScaleUpModule, SpatialTransformer, image_2d_distilled_transformer

__all__ = ["Net2DSeg"]


class Net2DSeg(nn.Module):
    def __init__(self, num_classes: int, dual_head: bool, backbone_2d_kwargs=dict()):
        super().__init__()
        kw = backbone_2d_kwargs
        self.stn_down = SpatialTransformer(in_channels=3)
        # channels lifted onto the points: the reference's literal 96; `stn_feat_channels` lets a test build a narrow model
        self.feat_channels = int(kw.get("stn_feat_channels", None) or 96)
        self.hidden_channels = 768   # ViT width

        if kw.get("middle_feat_block_number", None) is not None:
            self.middle_feat_block_number = str(kw["middle_feat_block_number"])
        else:
            self.middle_feat_block_number = None
        if kw.get("late_feat_block_number", None) is not None:
            self.late_feat_block_number = str(kw["late_feat_block_number"])
        else:
            self.late_feat_block_number = None

        # the backbone is built as in Net2DBillinear (image_models_billinear.py), minus the HIP graphs
        vit_kwargs = dict(remove_tokens_outputs=True)
        if kw.get("vit_depth", None) is not None:
            vit_kwargs["depth"] = int(kw["vit_depth"])
        if kw.get("skip_unused_blocks", True) and self.late_feat_block_number is not None:
            taps = [int(self.late_feat_block_number)] + ([int(self.middle_feat_block_number)] if self.middle_feat_block_number else [])
            vit_kwargs["last_block"] = max(taps)
        self.backbone = image_2d_distilled_transformer(pretrained=False, **vit_kwargs)
        if kw.get("IMAGE_PRETRAINED_PATH", "") != "":
            ckpt = torch.load(kw["IMAGE_PRETRAINED_PATH"], map_location="cpu", weights_only=True)["state_dict"]
            new_state_dict = OrderedDict((k.replace("backbone.", ""), v) for k, v in ckpt.items() if "backbone" in k)
            self.backbone.load_state_dict(new_state_dict)
        self.backbone.set_switches(kw)      # attn_impl, vit_bf16, vit_linear_impl, image_native_train, image_native_stems
        # parameters that can never receive a gradient: the final `norm` (forward_blocks never applies it) and blocks past the last tap
        for p in self.backbone.norm.parameters():
            p.requires_grad_(False)
        if self.backbone.last_block is not None:
            for i, blk in enumerate(self.backbone.blocks):
                if i > self.backbone.last_block:
                    for p in blk.parameters():
                        p.requires_grad_(False)

        self.up = nn.ModuleDict()
        if self.middle_feat_block_number:
            self.up[self.middle_feat_block_number] = ScaleUpModule(input_features=self.hidden_channels, output_features=self.feat_channels,
                                                                   kernel_size=16, stride=16)
        self.up[self.late_feat_block_number] = ScaleUpModule(input_features=self.hidden_channels, output_features=self.feat_channels,
                                                             kernel_size=16, stride=16)

        self.set_loc_impl(kw.get("stn_loc_impl", None) or "library")

        self.linear = nn.Linear(self.feat_channels, num_classes)
        self.dual_head = dual_head
        if dual_head:
            self.linear2 = nn.Linear(self.feat_channels, num_classes)

    def set_loc_impl(self, impl: str):
        """"library" | "ftx" for the localisation nets of `stn_down` and of every `up[*].up_stn` (SpatialTransformer.set_loc_impl)."""
        self.stn_down.set_loc_impl(impl)
        for m in self.up.values():
            m.up_stn.set_loc_impl(impl)
        self.stn_loc_impl = impl
        return self

    def set_native_train(self, on=True):
        """cfg.MODEL.image_native_train: every block of the trunk as one node of the native training executor (see the module docstring)."""
        self.backbone.set_native_train(on)
        return self

    def native_train_reason(self):
        """Why the last forward did not run the native training executor; None when it did."""
        return self.backbone.native_train_reason()

    def set_native_stems(self, on=True):
        """cfg.MODEL.image_native_stems: the patch embedding on the library's training forms (Image2DTransformer.set_native_stems); the
        resampled image carries a gradient here, so the embedding's backward also writes the image gradient through the fold."""
        self.backbone.set_native_stems(on)
        return self

    def native_stems_reason(self):
        """Why the last forward did not run the native patch embedding; None when it did."""
        return self.backbone.native_stems_reason()

    def get_img_feats(self, img_indices, block_id: str, image_shape: tuple, backbone_output: Dict):
        """reference image_models_stn.py:63-100 -> (sum N, feat_channels): the rows the reference picks out of the map that
        `self.up[block_id]` resamples to the image's (H, W)."""
        H, W = int(image_shape[-2]), int(image_shape[-1])
        x = backbone_output[block_id]
        B, N, EMBED_DIM = x.shape
        x = x.transpose(1, 2).reshape(B, EMBED_DIM, 384 // 16, 384 // 16)
        idx, frame = pack_img_indices(img_indices, x.device)
        return self.up[block_id].lift(x, idx, frame, H, W)

    def forward(self, img, img_indices):
        """reference image_models_stn.py:102-128."""
        img_indices = pack_img_indices(img_indices, img.device)
        x = self.stn_down(img, (self.feat_channels, 384, 384))
        backbone_output = self.backbone.forward_blocks(x)
        late_feats = self.get_img_feats(img_indices, self.late_feat_block_number, img.shape, backbone_output)
        x = spf.linear(late_feats, self.linear.weight, self.linear.bias)
        preds = {"img_feats": late_feats, "img_seg_logit": x}
        if self.dual_head:
            preds["img_seg_logit2"] = spf.linear(late_feats, self.linear2.weight, self.linear2.bias)
        if self.middle_feat_block_number:
            preds["img_middle_feats"] = self.get_img_feats(img_indices, self.middle_feat_block_number, img.shape, backbone_output)
        return preds
