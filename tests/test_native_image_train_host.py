"""Host side of the native training executor of the ViT image branch (include/ftx.h: ftx_vit_train_fwd / ftx_vit_train_bwd): the record
size, the arena size and every refusal answer without a GPU and before anything is launched; the eval executor, whose checker moved to
the header both share, refuses what it refused with the texts it had; the switch reaches the trunk and says why it does not engage."""
import numpy as np
import pytest
import torch

from fusiontransformer_amd import native_image as ni
from fusiontransformer_amd import native_image_train as nit
from tests.helpers import small_cfg
from tests.test_native_image_host import EINVAL, EWORKSPACE, FAKE, call as eval_call, err, tables


def grad_table(n_blocks):
    g = np.zeros(n_blocks, dtype=ni.BLOCK)
    for f in ni.BLOCK_FIELDS:
        g[f] = FAKE
    return g


def fwd(L, model, blocks, b=1, first=0, last=None, linear=0, attn=0, x=FAKE, out=FAKE, arena=FAKE, arena_bytes=1 << 40):
    last = len(blocks) - 1 if last is None else last
    return L.ftx_vit_train_fwd(ni._ptr(model), ni._ptr(blocks), len(blocks), b, x, first, last, linear, attn, out, arena, arena_bytes, None)


def bwd(L, model, blocks, grads, b=1, first=0, last=None, linear=0, attn=0, x=FAKE, gout=FAKE, gin=FAKE, arena=FAKE, arena_bytes=1 << 40):
    last = len(blocks) - 1 if last is None else last
    return L.ftx_vit_train_bwd(ni._ptr(model), ni._ptr(blocks), None if grads is None else ni._ptr(grads), len(blocks), b, x, gout, first, last, linear,
                               attn, gin, arena, arena_bytes, None)


def test_record_size_matches_the_numpy_dtype(ftx_lib):
    assert ftx_lib.ftx_vit_train_block_bytes() == ni.BLOCK.itemsize == 96
    nit.check_record_sizes()


def test_arena_bytes_grows_with_b_and_with_the_segment_and_depends_on_nothing_else(ftx_lib):
    model, blocks, _ = tables()
    by_b = [nit.arena_bytes(model, 3, 0, 2, b) for b in (1, 2, 3, 4, 8)]
    assert all(s % 256 == 0 and s > 0 for s in by_b) and all(b > a for a, b in zip(by_b, by_b[1:]))
    one, two, three = (nit.arena_bytes(model, 3, 0, last, 2) for last in (0, 1, 2))
    assert one < two < three
    assert nit.arena_bytes(model, 3, 1, 2, 2) == two and nit.arena_bytes(model, 3, 2, 2, 2) == one      # the count of blocks, not which
    assert nit.arena_bytes(model, 12, 1, 2, 2) == two                                                      # nor the table's length
    assert [nit.arena_bytes(model, 3, 0, 2, b) for b in (1, 2, 3, 4, 8)] == by_b
    rows = 2 * (2 + 24 * 24)
    # per block what the backward reads (8 token-sized tensors less the first block's s, pre and act), once the temporaries
    assert three >= 4 * rows * (3 * (8 * 768 + 2 * 3072) - 768 + 6 * 768 + 3072)
    assert ftx_lib.ftx_vit_train_arena_bytes(ni._ptr(model), 3, 0, 2, 0) >= 256
    bad, _, _ = tables(dim=700)
    assert ftx_lib.ftx_vit_train_arena_bytes(ni._ptr(bad), 3, 0, 2, 1) == 0 and err(ftx_lib).startswith("ftx_vit_train_arena_bytes:")
    assert ftx_lib.ftx_vit_train_arena_bytes(ni._ptr(model), 3, 1, 3, 1) == 0 and "blocks [1, 3] outside 0..2" in err(ftx_lib)
    with pytest.raises(RuntimeError, match="ftx_vit_train_arena_bytes"):
        nit.arena_bytes(bad, 3, 0, 2, 1)


REFUSALS = [
    ("heads", dict(heads=11), {}, "heads * 64 != dim"),
    ("dim", dict(dim=640, heads=10), {}, "dim 640"),
    ("hidden", dict(hidden=3000), {}, "hidden"),
    ("range past the table", dict(), dict(first=1, last=3), "blocks [1, 3] outside 0..2"),
    ("range reversed", dict(), dict(first=2, last=1), "blocks [2, 1]"),
    ("range negative", dict(), dict(first=-1, last=1), "blocks [-1, 1]"),
    ("linear mode", dict(), dict(linear=2), "linear_mode"),
    ("attention mode", dict(), dict(attn=3), "attn_mode"),
    ("attention mode negative", dict(), dict(attn=-1), "attn_mode"),
    ("arena alignment", dict(), dict(arena=FAKE + 16), "256-byte aligned"),
    ("null arena", dict(), dict(arena=None), "256-byte aligned"),
    ("null input", dict(), dict(x=None), "null x_in"),
    ("misaligned input", dict(), dict(x=FAKE + 4), "16-byte aligned"),
    ("batch", dict(), dict(b=-1), "batch -1"),
]


@pytest.mark.parametrize("entry", ["fwd", "bwd"])
@pytest.mark.parametrize("name,shape,how,text", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_both_directions_refuse_before_the_first_launch(ftx_lib, entry, name, shape, how, text):
    model, blocks, _ = tables(**shape)
    if entry == "fwd":
        rc = fwd(ftx_lib, model, blocks, **how)
    else:
        rc = bwd(ftx_lib, model, blocks, grad_table(len(blocks)), **how)
    assert rc == EINVAL, name
    msg = err(ftx_lib)
    assert msg.startswith("ftx_vit_train_%s:" % entry) and text in msg, msg


def test_null_and_misaligned_parameter_and_gradient_pointers(ftx_lib):
    model, blocks, _ = tables()
    grads = grad_table(3)
    for run, me in ((lambda: fwd(ftx_lib, model, blocks), "ftx_vit_train_fwd:"), (lambda: bwd(ftx_lib, model, blocks, grads), "ftx_vit_train_bwd:")):
        blocks["fc1_w"][1] = 0
        assert run() == EINVAL and err(ftx_lib).startswith(me) and "block 1: null parameter" in err(ftx_lib)
        blocks["fc1_w"][1] = FAKE
        blocks["qkv_b"][2] = FAKE + 8
        assert run() == EINVAL and "block 2: parameters must be 16-byte aligned" in err(ftx_lib)
        blocks["qkv_b"][2] = FAKE
    blocks["fc1_w"][0] = 0      # a record outside the segment is not read
    assert bwd(ftx_lib, model, blocks, grads, first=1) == EINVAL and "no forward" in err(ftx_lib)
    blocks["fc1_w"][0] = FAKE
    assert bwd(ftx_lib, model, blocks, None) == EINVAL and "null gradient table" in err(ftx_lib)
    for f in ni.BLOCK_FIELDS:      # every one of the twelve
        grads[f][1] = 0
        assert bwd(ftx_lib, model, blocks, grads) == EINVAL and "block 1: null gradient" in err(ftx_lib), f
        grads[f][1] = FAKE + 4
        assert bwd(ftx_lib, model, blocks, grads) == EINVAL and "block 1: gradients must be 16-byte aligned" in err(ftx_lib), f
        grads[f][1] = FAKE
    assert bwd(ftx_lib, model, blocks, grads, gout=None) == EINVAL and "null x_in, grad_out or grad_in" in err(ftx_lib)
    assert bwd(ftx_lib, model, blocks, grads, gin=FAKE + 8) == EINVAL and "16-byte aligned" in err(ftx_lib)
    assert fwd(ftx_lib, model, blocks, out=None) == EINVAL and "null x_in or x_out" in err(ftx_lib)


def test_small_arena_missing_forward_and_empty_batch(ftx_lib):
    model, blocks, _ = tables()
    grads = grad_table(3)
    need = nit.arena_bytes(model, 3, 0, 2, 2)
    for rc, me in ((fwd(ftx_lib, model, blocks, b=2, arena_bytes=need - 256), "ftx_vit_train_fwd:"),):
        assert rc == EWORKSPACE and err(ftx_lib).startswith(me) and "ftx_vit_train_arena_bytes" in err(ftx_lib)
    assert bwd(ftx_lib, model, blocks, grads, b=2, arena_bytes=need - 256) == EWORKSPACE
    assert err(ftx_lib).startswith("ftx_vit_train_bwd:") and "ftx_vit_train_arena_bytes" in err(ftx_lib)
    # a backward on an arena no forward ran on: refused on the host, with the call it misses
    assert bwd(ftx_lib, model, blocks, grads, b=2, linear=1, attn=2) == EINVAL
    assert "no forward of b = 2, blocks [0, 2], linear_mode 1, attn_mode 2 ran on this arena" in err(ftx_lib)
    assert ftx_lib.ftx_vit_train_release(FAKE) == 0 and ftx_lib.ftx_vit_train_release(None) == 0      # nothing noted: a no-op
    # an empty batch is a no-op that touches no arena and needs no forward
    assert fwd(ftx_lib, model, blocks, b=0, x=None, out=None, arena=None, arena_bytes=0) == 0
    assert bwd(ftx_lib, model, blocks, grads, b=0, x=None, gout=None, gin=None, arena=None, arena_bytes=0) == 0
    assert bwd(ftx_lib, model, blocks, grads, b=1) == EINVAL and "no forward" in err(ftx_lib)      # and leaves no note behind


def test_the_eval_entry_refuses_what_it_refused_with_the_same_texts(ftx_lib):
    """The texts of tests/test_native_image_host.py, spelled out in full: the checker moved, the messages did not."""
    cases = [
        (dict(heads=11), {}, "ftx_vit_eval: heads * 64 != dim (heads=11 dim=768)"),
        (dict(dim=640, heads=10), {}, "ftx_vit_eval: dim 640 is not one the LayerNorm kernel takes (256, 512, 768, 1024)"),
        (dict(hidden=3000), {}, "ftx_vit_eval: hidden must be a multiple of 64 (hidden=3000)"),
        (dict(), dict(first=2, last=1, n_taps=0), "ftx_vit_eval: blocks [2, 1] outside 0..2"),
        (dict(), dict(linear=2), "ftx_vit_eval: linear_mode must be 0 (split) or 1 (bf16)"),
        (dict(), dict(attn=-1), "ftx_vit_eval: attn_mode must be 0 (fp32), 1 (bf16) or 2 (split)"),
        (dict(), dict(b=-1), "ftx_vit_eval: batch -1 outside [0, 4096]"),
        (dict(n_blocks=65), {}, "ftx_vit_eval: block count 65 outside [1, 64]"),
    ]
    for shape, how, text in cases:
        model, blocks, taps = tables(**shape)
        assert eval_call(ftx_lib, model, blocks, taps, **how) == EINVAL and err(ftx_lib) == text, (text, err(ftx_lib))
    model, blocks, taps = tables()
    blocks["norm2_b"][1] = 0
    assert eval_call(ftx_lib, model, blocks, taps) == EINVAL and err(ftx_lib) == "ftx_vit_eval: block 1: null parameter"
    blocks["norm2_b"][1] = FAKE + 4
    assert eval_call(ftx_lib, model, blocks, taps) == EINVAL and err(ftx_lib) == "ftx_vit_eval: block 1: parameters must be 16-byte aligned"
    blocks["norm2_b"][1] = FAKE
    assert ftx_lib.ftx_vit_eval_arena_bytes(ni._ptr(tables(dim=700)[0]), 3, 1) == 0
    assert err(ftx_lib) == "ftx_vit_eval_arena_bytes: dim 700 is not one the LayerNorm kernel takes (256, 512, 768, 1024)"
    assert eval_call(ftx_lib, model, blocks, taps, b=0, arena=None, arena_bytes=0) == 0


def test_gradient_layout_keeps_the_layernorm_groups_together():
    where, total = nit.grad_layout(1, 3, 256, 1024)
    assert sorted(where) == sorted((i, f) for i in (1, 2, 3) for f in ni.BLOCK_FIELDS)
    spans = sorted((off, off + int(np.prod(shape))) for off, shape in where.values())
    assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))      # no gap, no overlap
    assert all(off % 4 == 0 for off, _ in where.values())                                                          # 16-byte aligned
    for i in (1, 2, 3):
        assert where[(i, "norm2_b")][0] == where[(i, "norm2_w")][0] + 256 and where[(i, "proj_b")][0] == where[(i, "norm2_b")][0] + 256
        assert where[(i, "norm1_b")][0] == where[(i, "norm1_w")][0] + 256
        if i > 1:
            assert where[(i - 1, "fc2_b")][0] == where[(i, "norm1_b")][0] + 256
    assert where[(2, "fc1_w")][1] == (1024, 256) and where[(2, "fc2_w")][1] == (256, 1024) and where[(2, "qkv_w")][1] == (768, 256)


def test_the_switch_reaches_the_trunk_and_says_why_it_does_not_engage():
    from fusiontransformer_amd.models.build import build_model
    cfg = small_cfg("late")
    torch.manual_seed(0)
    net = build_model(cfg)[0].image_backbone
    bb = net.backbone
    assert bb.image_native_train is False and net.native_train_reason() == "the switch is off"
    img = torch.zeros(1, 3, 8, 8)
    assert bb._native_trainer(img) is None and bb.native_train_reason() == "the switch is off"
    net.set_native_train(True)
    assert bb.image_native_train is True
    assert bb._native_trainer(img) is None and "not a float32 tensor on the GPU" in net.native_train_reason()
    with torch.no_grad():
        assert bb._native_trainer(img) is None and net.native_train_reason() == "gradients are disabled"
    net.eval()
    assert bb._native_trainer(img) is None and net.native_train_reason() == "eval mode"
    net.set_native_train(False)
    assert bb._native_trainer(img) is None and net.native_train_reason() == "the switch is off"
    cfg.MODEL.image_native_train = True
    assert build_model(cfg)[0].image_backbone.backbone.image_native_train is True
    from fusiontransformer_amd import config
    from fusiontransformer_amd.models.build import build_image_model
    stn = config.image_stn_cfg()
    stn.MODEL.vit_depth, stn.MODEL.late_feat_block_number, stn.MODEL.stn_feat_channels = 2, 1, 8
    assert build_image_model(stn)[0].image_backbone.backbone.image_native_train is False
    stn.MODEL.image_native_train = True
    seg = build_image_model(stn)[0].image_backbone
    assert seg.backbone.image_native_train is True and seg.native_train_reason() == "the switch is off"


def test_model_record_and_trunk_modes_of_a_bare_trunk():
    from fusiontransformer_amd.models.transformers import Image2DTransformer
    torch.manual_seed(0)
    bb = Image2DTransformer(img_size=96, embed_dim=256, depth=2, num_heads=4)
    m = nit.model_record(bb, 38)[0]
    assert (m["dim"], m["heads"], m["hidden"], m["grid"], m["t0"], m["patch"], m["in_chans"]) == (256, 4, 1024, 6, 2, 16, 3)
    with pytest.raises(nit.Unsupported, match="square grid"):
        nit.model_record(bb, 40)
    with pytest.raises(nit.Unsupported, match="library"):
        ni.trunk_modes(bb)
    bb.set_linear_impl("ftx_split")
    bb.set_attention_impl("ftx_split")
    assert ni.trunk_modes(bb) == (ni.LINEAR_SPLIT, ni.ATTN_SPLIT)
    keep = []
    blocks = ni.block_table(bb, ni.keeper(keep))
    assert len(blocks) == 2 and len(keep) == 24
    assert [int(blocks[1][f]) for f in ni.BLOCK_FIELDS] == [t.data_ptr() for t in ni.block_tensors(bb.blocks[1])]
