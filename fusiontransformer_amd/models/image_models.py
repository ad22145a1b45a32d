"""ImageSeg and ImageSegBilinear: mirror of FusionTransformer/models/image_models.py:8-36, the two image-only baselines.

`ImageSeg` brings the picture to the ViT and back with learned affine resampling (image_models_stn.py); `ImageSegBilinear` uses
fixed nearest resampling for the same job (image_models_billinear.py)."""
import torch.nn as nn

from .image_models_billinear import Net2DBillinear
from .image_models_stn import Net2DSeg


class ImageSeg(nn.Module):
    def __init__(self, num_classes, dual_head, backbone_2d_kwargs):
        super(ImageSeg, self).__init__()
        self.image_backbone = Net2DSeg(num_classes=num_classes, dual_head=dual_head, backbone_2d_kwargs=backbone_2d_kwargs)
        bb = self.image_backbone
        # this model returns the main head only (image_models.py:18-20): what feeds nothing but the other outputs never receives a
        # gradient, its .grad stays None in the reference and the optimizer skips it; frozen like the trunk's unused parameters
        unused = [bb.linear2] if dual_head else []
        if bb.middle_feat_block_number and bb.middle_feat_block_number != bb.late_feat_block_number:
            unused.append(bb.up[bb.middle_feat_block_number])
        for mod in unused:
            for p in mod.parameters():
                p.requires_grad_(False)

    def forward(self, data_dict):
        preds_image = self.image_backbone(data_dict["img"], data_dict["img_indices"])
        return {"img_seg_logit": preds_image["img_seg_logit"]}


class ImageSegBilinear(nn.Module):
    def __init__(self, num_classes, dual_head, backbone_2d_kwargs):
        super(ImageSegBilinear, self).__init__()
        self.image_backbone = Net2DBillinear(num_classes=num_classes, dual_head=dual_head, backbone_2d_kwargs=backbone_2d_kwargs)
        if dual_head:
            # this model returns the main head only (image_models.py:35-36): the second head never receives a gradient, its
            # .grad stays None in the reference and the optimizer skips it; frozen like the trunk's unused parameters
            for p in self.image_backbone.linear2.parameters():
                p.requires_grad_(False)

    def forward(self, data_dict):
        preds_image = self.image_backbone(data_dict["img"], data_dict["img_indices"], lift_size=data_dict.get("lift_size"))
        return {"img_seg_logit": preds_image["img_seg_logit"]}
