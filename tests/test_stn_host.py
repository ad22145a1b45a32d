"""The spatial-transformer image model without a GPU: the float64 restatement (tests/stn_ref.py) against the reference's own modules
(tests/golden/stn.npz), the module trees against the reference's names, and the dispatch."""
import os

import numpy as np
import pytest
import torch

from tests import stn_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stn.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _params(golden, tag, requires_grad=False):
    return {str(n): torch.from_numpy(golden["%s_param_%s" % (tag, n)]).double().requires_grad_(requires_grad) for n in golden[tag + "_names"]}


def test_restatement_equals_the_reference_spatial_transformer(golden):
    p = _params(golden, "st", True)
    x = torch.from_numpy(golden["st_x"]).requires_grad_(True)
    y = R.spatial_transformer(p, "", x, (24, 24))
    assert (y.detach() - torch.from_numpy(golden["st_y"])).abs().max().item() <= 1e-12
    assert (R.theta_of(p, "", x).detach() - torch.from_numpy(golden["st_theta"])).abs().max().item() <= 1e-12
    (y * torch.from_numpy(golden["st_g"])).sum().backward()
    assert (x.grad - torch.from_numpy(golden["st_grad_x"])).abs().max().item() <= 1e-12
    for n, t in p.items():
        assert (t.grad - torch.from_numpy(golden["st_grad_" + n])).abs().max().item() <= 1e-12, n
    # the case means something: non-identity theta, samples inside and outside the source
    th = golden["st_theta"]
    assert np.abs(th - np.array([[1, 0, 0], [0, 1, 0]])).max() > 0.05 and np.abs(golden["st_grad_fc_loc.2.bias"]).min() > 0


def test_restatement_equals_the_reference_scale_up_module(golden):
    p = _params(golden, "su", True)
    x = torch.from_numpy(golden["su_x"]).requires_grad_(True)
    H, W = (int(v) for v in golden["su_size"])
    idx, frame = torch.from_numpy(golden["su_idx"]), torch.from_numpy(golden["su_frame"])
    with torch.no_grad():
        dense = R.scale_up(p, "", x, (H, W), 4)
    assert (dense - torch.from_numpy(golden["su_dense"])).abs().max().item() <= 1e-12
    assert (R.pick(dense, idx, frame) - torch.from_numpy(golden["su_feats"])).abs().max().item() <= 1e-12
    feats = R.scale_up_points(p, "", x, idx, frame, H, W, 4)
    assert (feats.detach() - torch.from_numpy(golden["su_feats"])).abs().max().item() <= 1e-12
    (feats * torch.from_numpy(golden["su_g"])).sum().backward()
    assert (x.grad - torch.from_numpy(golden["su_grad_x"])).abs().max().item() <= 1e-12
    for n, t in p.items():
        assert (t.grad - torch.from_numpy(golden["su_grad_" + n])).abs().max().item() <= 1e-12, n


def test_closed_form_equals_torch_in_float64_inside_and_outside():
    g = torch.Generator().manual_seed(3)
    src = torch.randn((2, 3, 23, 37), generator=g, dtype=torch.float64)
    for kind in ("identity", "scale", "rotate", "flip", "outside"):
        th = R.theta_case(kind, 2, np.random.default_rng(5)).double()
        want = R.torch_dense(src, th, (33, 65))
        assert (R.sample(src, th, (33, 65)) - want).abs().max().item() <= 1e-13, kind
        if kind == "outside":
            assert want.abs().max().item() == 0
    idx = torch.stack([torch.randint(0, 33, (300,), generator=g), torch.randint(0, 65, (300,), generator=g)], 1)
    frame = torch.randint(0, 2, (300,), generator=g).int()
    th = R.theta_case("rotate", 2).double()
    a, b = R.sample_points(src, th, idx, frame, 33, 65), R.torch_points(src, th, idx, frame, 33, 65)
    assert (a - b).abs().max().item() <= 1e-13 and (a - R.pick(R.sample(src, th, (33, 65)), idx, frame)).abs().max().item() <= 1e-13


def test_module_trees_equal_the_reference_names_and_shapes(golden):
    from fusiontransformer_amd.models.transformers import ScaleUpModule, SpatialTransformer
    for tag, mod in (("st", SpatialTransformer(3)), ("su", ScaleUpModule(16, 8, 4, 4))):
        names = [str(n) for n in golden[tag + "_names"]]
        assert [n for n, _ in mod.named_parameters()] == names and list(mod.state_dict().keys()) == names
        for n, p in mod.named_parameters():
            assert tuple(p.shape) == golden["%s_param_%s" % (tag, n)].shape, n
    st = SpatialTransformer(5)
    assert st.fc_loc[2].weight.abs().max().item() == 0
    assert st.fc_loc[2].bias.tolist() == [1, 0, 0, 0, 1, 0]
    assert ScaleUpModule(16, 8, 4, 4).up_stn.fc_loc[2].bias.tolist() == [1, 0, 0, 0, 1, 0]


def test_modules_on_the_host_equal_the_golden(golden):
    """The module code around the kernels (localisation net, the up-convolution as a GEMM, the layout) on the CPU, float64."""
    from fusiontransformer_amd.models.transformers import ScaleUpModule, SpatialTransformer
    st = SpatialTransformer(3).double()
    st.load_state_dict({str(n): torch.from_numpy(golden["st_param_" + str(n)]).double() for n in golden["st_names"]})
    x = torch.from_numpy(golden["st_x"])
    assert (st.theta(x) - torch.from_numpy(golden["st_theta"])).abs().max().item() <= 1e-12
    assert (st(x, (3, 24, 24)) - torch.from_numpy(golden["st_y"])).abs().max().item() <= 1e-12
    su = ScaleUpModule(16, 8, 4, 4).double()
    su.load_state_dict({str(n): torch.from_numpy(golden["su_param_" + str(n)]).double() for n in golden["su_names"]})
    x = torch.from_numpy(golden["su_x"])
    assert (su.up(x) - su.up_conv(x)).abs().max().item() <= 1e-12          # one GEMM + permute == the transposed convolution
    assert (su(x, (8, 30, 44)) - torch.from_numpy(golden["su_dense"])).abs().max().item() <= 1e-12


def _model_cfg(**kw):
    from fusiontransformer_amd.config import image_stn_cfg
    cfg = image_stn_cfg()
    cfg.MODEL.vit_depth, cfg.MODEL.late_feat_block_number = 2, 1
    for k, v in kw.items():
        cfg.MODEL[k] = v
    return cfg


def test_net2dseg_keys_and_frozen_parameters():
    from fusiontransformer_amd.models.build import build_image_model
    from fusiontransformer_amd.models.image_models import ImageSeg
    cfg = _model_cfg(DUAL_HEAD=True, middle_feat_block_number=0, stn_feat_channels=8)
    model, metric = build_image_model(cfg)
    assert isinstance(model, ImageSeg) and metric.name == "seg_iou_2d"
    keys = set(model.state_dict().keys())
    prefixes = ("image_backbone.stn_down.localization.0.", "image_backbone.stn_down.fc_loc.2.", "image_backbone.backbone.blocks.1.",
                "image_backbone.backbone.patch_embed.proj.", "image_backbone.up.0.up_conv.", "image_backbone.up.1.up_conv.",
                "image_backbone.up.1.up_stn.localization.3.", "image_backbone.up.1.up_stn.fc_loc.0.", "image_backbone.linear.",
                "image_backbone.linear2.")
    for pre in prefixes:
        assert any(k.startswith(pre) for k in keys), pre
    assert not any("sample_down" in k for k in keys)
    bb = model.image_backbone
    assert bb.feat_channels == 8 and bb.up["1"].up_conv.weight.shape == (768, 8, 16, 16) and bb.linear.weight.shape == (20, 8)
    assert bb.backbone.graph_taps is None                                 # the trunk runs eagerly in this model
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    assert frozen == {n for n, _ in model.named_parameters()
                      if n.startswith(("image_backbone.backbone.norm.", "image_backbone.linear2.", "image_backbone.up.0."))}
    # the reference's width by default, and a single head keeps every used parameter trainable
    full, _ = build_image_model(_model_cfg())
    assert full.image_backbone.feat_channels == 96 and full.image_backbone.up["1"].up_conv.weight.shape == (768, 96, 16, 16)
    assert {n for n, p in full.named_parameters() if not p.requires_grad} == {"image_backbone.backbone.norm.weight", "image_backbone.backbone.norm.bias"}


def test_build_model_builds_imageseg_only_behind_the_switch():
    from fusiontransformer_amd.config import get_cfg_defaults, image_cfg, image_stn_cfg
    from fusiontransformer_amd.models.build import build_image_model, build_model
    assert get_cfg_defaults().MODEL.image_stn is False and image_stn_cfg().MODEL.image_stn is True
    cfg = _model_cfg()
    model, metric = build_model(cfg)
    assert type(model).__name__ == "ImageSeg" and type(model.image_backbone).__name__ == "Net2DSeg"
    cfg.MODEL.image_stn = False
    with pytest.raises(NotImplementedError) as err:
        build_model(cfg)
    assert "image_stn" in str(err.value) and "build_image_model" in str(err.value)
    assert type(build_image_model(cfg)[0]).__name__ == "ImageSeg"          # the direct builder does not look at the switch
    plain = image_cfg()
    plain.MODEL.TYPE = "ImageSeg"
    with pytest.raises(NotImplementedError):
        build_model(plain)


def test_trainstep_takes_the_model_in_image_mode():
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    cfg = _model_cfg(stn_feat_channels=8)
    cfg.OPTIMIZER.TYPE = "SGD"
    model, metric = build_model(cfg)
    step = TrainStep(cfg, model, metrics=metric)
    assert step.mode == "image" and len(step.metrics) == 1
    assert len(step.optimizer.param_groups[0]["params"]) == sum(p.requires_grad for p in model.parameters())


def test_operand_validation_answers_before_any_launch():
    from fusiontransformer_amd import functional as spf
    src, th = torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 3)
    with pytest.raises(ValueError):
        spf.affine_sample(src, th, (4, 4))                                 # not on the device: there is no CPU fallback
    with pytest.raises(ValueError):
        spf.affine_lift(src, th, torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 4, 4)
    with pytest.raises(ValueError):
        spf.affine_sample(src, th, (0, 4))
    with pytest.raises(RuntimeError):
        spf.affine_sample(src.requires_grad_(True), th, (4, 4))           # the dense form has no gradient for src


def test_library_checks_arguments_without_a_gpu(ftx_lib):
    import ctypes
    strides = (ctypes.c_int64 * 4)(48, 16, 4, 1)
    assert ftx_lib.ftx_affine_theta_workspace_bytes(2) == 8 * 1024 * 12 and ftx_lib.ftx_affine_theta_workspace_bytes(129) == 0
    assert ftx_lib.ftx_affine_sample_fwd(None, strides, 0, 3, 4, 4, None, 4, 4, None, None) == -1
    assert b"bad source size" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_affine_sample_fwd(None, strides, 1, 3, 4, 4, None, 4, 4, None, None) == -1
    assert b"null pointer" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_affine_lift_fwd(None, strides, 1, 3, 4, 4, None, None, None, 0, 4, 4, None, None) == 0      # no points: a no-op
    assert ftx_lib.ftx_affine_lift_cells(None, None, None, 5, 1, 40000, 4, 4, 4, None, None) == -1
    assert b"too large" in ftx_lib.ftx_last_error()
    bad = (ctypes.c_int64 * 4)(48, 16, -4, 1)
    assert ftx_lib.ftx_affine_sample_bwd_theta(None, bad, 1, 3, 4, 4, None, None, 4, 4, None, None, 0, None) == -1
    assert b"negative stride" in ftx_lib.ftx_last_error()
