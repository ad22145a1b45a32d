"""Host side of the fused localisation-net path: the configuration key and its way to the modules, the restatement tests/loc_ref.py
against tests/stn_ref.py, the ambiguity caps of every GPU case, and the "ftx" setting on CPU tensors.  No GPU."""
import pytest
import torch

from tests import loc_ref as LR
from tests import stn_ref as R


def _cfg(**kw):
    from fusiontransformer_amd.config import image_stn_cfg
    cfg = image_stn_cfg()
    cfg.MODEL.vit_depth, cfg.MODEL.late_feat_block_number, cfg.MODEL.stn_feat_channels = 2, 1, 8
    for k, v in kw.items():
        cfg.MODEL[k] = v
    return cfg


def _transformers(net):
    return [net.stn_down] + [m.up_stn for m in net.up.values()]


def test_config_default_and_pass_through():
    from fusiontransformer_amd.config import get_cfg_defaults, image_stn_cfg
    from fusiontransformer_amd.models.build import build_image_model
    assert image_stn_cfg().MODEL.stn_loc_impl == "library"
    assert "stn_loc_impl" not in get_cfg_defaults().MODEL          # only the spatial-transformer configuration carries the key
    model, _ = build_image_model(_cfg())
    net = model.image_backbone
    assert net.stn_loc_impl == "library" and all(st.loc_impl == "library" for st in _transformers(net))
    keys = list(model.state_dict())
    model, _ = build_image_model(_cfg(stn_loc_impl="ftx", middle_feat_block_number=0))
    net = model.image_backbone
    assert len(net.up) == 2
    assert net.stn_loc_impl == "ftx" and all(st.loc_impl == "ftx" for st in _transformers(net))
    net.set_loc_impl("library")
    assert all(st.loc_impl == "library" for st in _transformers(net))
    model, _ = build_image_model(_cfg(stn_loc_impl="ftx"))
    assert list(model.state_dict()) == keys                         # the parameters stay in the nn.Conv2d modules


def test_an_unknown_value_raises():
    from fusiontransformer_amd.models.build import build_image_model
    from fusiontransformer_amd.models.transformers import SpatialTransformer
    with pytest.raises(ValueError):
        SpatialTransformer(3).set_loc_impl("miopen")
    with pytest.raises(ValueError):
        build_image_model(_cfg(stn_loc_impl="fused"))
    model, _ = build_image_model(_cfg())
    with pytest.raises(ValueError):
        model.image_backbone.set_loc_impl("")


def _module(seed, c):
    from fusiontransformer_amd.models.transformers import SpatialTransformer
    torch.manual_seed(seed)
    mod = SpatialTransformer(c)
    with torch.no_grad():
        mod.fc_loc[2].weight.copy_(torch.randn(mod.fc_loc[2].weight.shape) * 0.02)
    return mod


def test_loc_ref_is_stn_refs_chain():
    mod = _module(5, 3)
    p64 = {k: v.double() for k, v in mod.state_dict().items()}
    for shape in ((2, 3, 48, 80), (1, 3, 33, 31)):       # even and odd conv sizes: a dropped row and column
        x = torch.randn(shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
        assert torch.equal(LR.theta_of(p64, "", x), R.theta_of(p64, "", x))
    # the routed restatement with a layer's own routing is the layer, bit for bit, and its positions are the pool's
    x, w, bias = (t.double() for t in LR.inputs((2, 3, 9, 12, 7, 8)))
    y, sel = LR.layer(x, w, bias)
    assert torch.equal(LR.routed(x, w, bias, sel), y)
    assert sel.dtype == torch.int8 and int(sel.min()) >= -1 and int(sel.max()) <= 3 and bool(((sel == -1) == (y == 0)).all())
    win = LR.windows(torch.nn.functional.conv2d(x, w, bias))
    assert torch.equal(win.max(-1).values.clamp(min=0), y)
    # a tie goes to the first position in row-major order, a dead window to -1
    one = torch.ones((1, 1, 8, 8), dtype=torch.float64)
    wt = torch.zeros((8, 1, 7, 7), dtype=torch.float64)
    wt[:4, 0, 0, 0] = 1.0
    wt[4:, 0, 0, 0] = -1.0
    y, sel = LR.layer(one, wt, None)
    assert sel.view(-1).tolist() == [0, 0, 0, 0, -1, -1, -1, -1] and y.view(-1).tolist() == [1.0] * 4 + [0.0] * 4


@pytest.mark.parametrize("shape", sorted({s for s, _ in LR.SMALL}) + LR.FULL)
def test_ambiguity_caps(shape):
    """Under 0.5 % of the windows of every GPU case are ambiguous (the comparison of sel leaves only those out), and the float32
    yardstick itself routes like the truth outside them."""
    cs = LR.case(shape)
    print("loc %s: forward bar %.3e, ambiguous %.4f %% of %d windows" % (shape, cs["bar"], 100 * cs["ambiguous_share"], cs["ambiguous"].numel()))
    assert cs["bar"] > 0
    assert cs["ambiguous_share"] < LR.AMBIGUOUS_CAP
    assert not bool(((cs["yard_sel"] != cs["sel"]) & ~cs["ambiguous"]).any())


def test_ftx_on_cpu_tensors_is_todays_result():
    mod = _module(7, 8)
    x = torch.randn((2, 8, 40, 56), generator=torch.Generator().manual_seed(8))
    want_theta, want = mod.theta(x), mod(x, (8, 24, 24))
    mod.set_loc_impl("ftx")
    assert torch.equal(mod.theta(x), want_theta) and torch.equal(mod(x, (8, 24, 24)), want)
    assert list(mod.state_dict()) == list(_module(7, 8).state_dict())


def test_functional_refuses_cpu_tensors():
    from fusiontransformer_amd import functional as spf
    x, w, bias = LR.inputs((1, 3, 9, 12, 7, 8))
    with pytest.raises(ValueError):
        spf.loc_conv_pool_relu(x, w, bias)
