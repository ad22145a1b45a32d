"""The split attention scheme (attn_impl="ftx_split": every MFMA operand in three bf16 pieces, six piece products) against the bars of
the fp32 kernels, on the CPU: tests/attn_split_ref.emulate_split stands in for the kernels, attn_ref.Case(...).bars are the bars of
tests/test_attn_fp32_gpu.py, unchanged -- no tolerance in this file is a number.  The correct scheme is inside them at every shape and
key split; each cheaper scheme is outside them.  Then the model layer: the switch reaches every block, the graph keys and the native
executor's mode, and leaves the Linears' switches alone."""
import functools

import pytest
import torch

from tests import attn_ref as R
from tests import attn_split_ref as S

B, H, SCALE = 1, 2, 0.125
INSIDE = ([(kind, T) for kind in ("gauss", "peaked") for T in (1, 33, 129, 578)] +
          [("large", 578), ("ascending", 290), ("late_max", 290)])
# Every fault is outside the bars on all three (measured worst ratio at key split 2, in this order: five_products 2.0 / 1.4 / 1.5,
# three_products 2.5 / 3.9 / 3.2, p_one_piece 595 / 122 / 92, ds_one_piece 129 / 14 / 14, do_rounded 597 / 162 / 115): no case is dropped
# for any fault.
REJECTED = [("gauss", 129), ("peaked", 129), ("peaked", 578)]


@functools.lru_cache(maxsize=None)
def case(kind, T):
    return R.Case(kind, B, T, H, SCALE)


@pytest.mark.parametrize("split", [1, 2, 4])
@pytest.mark.parametrize("kind,T", INSIDE)
def test_six_products_are_inside_the_fp32_bars(kind, T, split):
    c = case(kind, T)
    r, E = c.ratios(S.emulate_split(c.qkv, c.go, SCALE, split))
    print(R.format_row(f"split emulation {kind} T={T} groups={split}", c.E32, E, r))
    assert R.worst(r) <= 1.0, (r, E)


def test_backward_groups_may_differ_from_the_forward():
    """The automatic choice: 8 key groups forward, 4 groups backward."""
    c = case("peaked", 578)
    r, E = c.ratios(S.emulate_split(c.qkv, c.go, SCALE, 8, bwd_split=4))
    assert R.worst(r) <= 1.0, (r, E)


@pytest.mark.parametrize("kind,T", REJECTED)
@pytest.mark.parametrize("fault", list(S.FAULTS))
def test_every_cheaper_scheme_is_outside_the_bars(fault, kind, T):
    c = case(kind, T)
    r, E = c.ratios(S.emulate_split(c.qkv, c.go, SCALE, 2, fault))
    print(R.format_row(f"{fault} {kind} T={T}", c.E32, E, r))
    assert R.worst(r) > 1.0, (fault, r)


def test_pieces_are_the_split_of_split_ref():
    from tests import split_ref
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * torch.logspace(-20, 20, 4096)
    x[:3] = torch.tensor([float("inf"), -float("inf"), 0.0])
    for a, b in zip(S.split3(x.numpy()), split_ref.split3(x)):
        assert torch.equal(torch.from_numpy(a), b)


# ---------------------------------------------------------------- functional and model layer
def test_operand_mode_names_the_split_and_refuses_a_contradiction():
    from fusiontransformer_amd import functional as spf
    assert spf.operand_mode(False, "split") == spf.SPLIT
    assert set(spf._ATTENTION) == {spf.FP32, spf.BF16, spf.SPLIT}
    assert spf._ATTENTION[spf.SPLIT] == ("ftx_attn_fwd_split", "attn_fwd_split", "ftx_attn_bwd_split", "attn_bwd_split")
    with pytest.raises(ValueError, match="contradicts"):
        spf.operand_mode(True, "split")
    with pytest.raises(ValueError, match="contradicts"):
        spf.attention(torch.zeros(1, 4, 3, 1, 64), 0.125, bf16=True, operands="split")


def _image_branch():
    from fusiontransformer_amd.models.build import build_model
    from tests.helpers import small_cfg
    torch.manual_seed(0)
    return build_model(small_cfg("middle"))[0].image_backbone


def test_attention_module_routes_the_mode(monkeypatch):
    """Attention.forward hands functional.attention the operand mode its attn_impl names."""
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.models import transformers as T
    assert T.ATTN_OPERANDS == {"ftx": "fp32", "ftx_bf16": "bf16", "ftx_split": "split"}
    seen = []

    def stub(qkv, scale, tiling=(0, 0), bf16=False, operands=None):
        seen.append(spf.operand_mode(bf16, operands))
        return qkv.new_zeros(qkv.shape[0], qkv.shape[1], qkv.shape[3] * qkv.shape[4])
    monkeypatch.setattr(spf, "attention", stub)
    att = _image_branch().backbone.blocks[0].attn
    assert att.attn_impl == "ftx", "the default stays the exact-fp32 kernels"
    x = torch.zeros(1, 5, 768)
    for impl, mode in (("ftx", spf.FP32), ("ftx_bf16", spf.BF16), ("ftx_split", spf.SPLIT)):
        att.attn_impl = impl
        att(x)
        assert seen.pop() == mode and not seen, impl


def test_switch_reaches_every_block_the_graph_keys_and_the_executor(monkeypatch):
    from fusiontransformer_amd import native_image as ni
    from fusiontransformer_amd.models import transformers as T
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)   # the keys record the device; no GPU is touched here
    net = _image_branch()
    b = net.backbone
    b.set_linear_impl("ftx_split")
    ex = ni.NativeImage(net)
    x = torch.zeros(1, 3, 384, 384)
    keys = lambda: (b._graph_key(x), b._infer_key(x), ex._signature())
    linears = lambda: [T.linear_switches(lin) for blk in b.blocks for lin in T.block_linears(blk)]
    base, lin0 = keys(), linears()
    assert ni.modes(net) == (ni.LINEAR_SPLIT, ni.ATTN_FP32)
    b.set_attention_impl("ftx_split")
    assert [blk.attn.attn_impl for blk in b.blocks] == ["ftx_split"] * len(b.blocks)
    assert [T.block_switches(blk)[0] for blk in b.blocks] == ["ftx_split"] * len(b.blocks)
    assert [new != old for new, old in zip(keys(), base)] == [True] * 3
    assert linears() == lin0, "the Linears' switches are not the attention's"
    assert ni.ATTN_SPLIT == 2 and ni.modes(net) == (ni.LINEAR_SPLIT, ni.ATTN_SPLIT)
    b.blocks[0].attn.attn_impl = "ftx"
    with pytest.raises(ni.Unsupported, match="attn_impl"):
        ni.modes(net)
    b.set_attention_impl("ftx")
    assert keys() == base
    # the other two ways in: set_switches (an image model's backbone_2d_kwargs) and cfg.MODEL.attn_impl through build_model
    b.set_switches({"attn_impl": "ftx_split"})
    assert all(blk.attn.attn_impl == "ftx_split" for blk in b.blocks) and linears() != lin0      # vit_linear_impl defaulted to "library"
    b.set_switches({})
    assert all(blk.attn.attn_impl == "ftx" for blk in b.blocks)


def test_cfg_and_build_kwarg_reach_the_blocks():
    from fusiontransformer_amd.models.build import build_model
    from tests.helpers import small_cfg
    cfg = small_cfg("middle")
    cfg.MODEL.attn_impl = "ftx_split"
    torch.manual_seed(0)
    vit = build_model(cfg)[0].image_backbone.backbone
    assert all(blk.attn.attn_impl == "ftx_split" for blk in vit.blocks)
