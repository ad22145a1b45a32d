"""Host side of the native eval executor of the ViT image branch (include/ftx.h: ftx_vit_patch_embed_*, ftx_vit_tap_stem_*,
ftx_rows_add_bias, ftx_vit_eval): record layouts, the arena size and every refusal answer without a GPU and before anything is
launched; `emit` writes the tables from a module tree."""
import ctypes

import numpy as np
import pytest
import torch

from fusiontransformer_amd import native_image as ni
from tests.helpers import small_cfg

FAKE = 0x10000   # a 256-byte aligned address that is never dereferenced: every call below is refused on the host
EINVAL, EWORKSPACE = -1, -3


def err(L):
    return L.ftx_last_error().decode()


def test_record_sizes_match_the_numpy_dtypes(ftx_lib):
    assert ftx_lib.ftx_vit_model_bytes() == ni.MODEL.itemsize == 72
    assert ftx_lib.ftx_vit_block_bytes() == ni.BLOCK.itemsize == 96
    assert ftx_lib.ftx_vit_tap_bytes() == ni.TAP.itemsize == 64
    ni.check_record_sizes()
    assert ftx_lib.ftx_version() >= 102


def tables(dim=768, heads=12, hidden=3072, n_blocks=3, tap_blocks=(0, 2), co=96):
    model = np.zeros(1, dtype=ni.MODEL)
    m = model[0]
    for f in ("patch_w", "patch_b", "cls", "dist", "pos"):
        m[f] = FAKE
    m["dim"], m["heads"], m["hidden"], m["patch"], m["grid"], m["t0"], m["in_chans"], m["eps"] = dim, heads, hidden, 16, 24, 2, 3, 1e-6
    blocks = np.zeros(n_blocks, dtype=ni.BLOCK)
    for f in ni.BLOCK_FIELDS:
        blocks[f] = FAKE
    taps = np.zeros(len(tap_blocks), dtype=ni.TAP)
    for f in ("stem_w", "stem_b", "gamma", "beta", "mean", "var"):
        taps[f] = FAKE
    taps["block"], taps["co"], taps["eps"] = list(tap_blocks), co, 1e-5
    return model, blocks, taps


def call(L, model, blocks, taps, b=1, first=0, last=None, linear=0, attn=0, arena=FAKE, arena_bytes=1 << 40, img=FAKE, n_taps=None, tap_out=FAKE):
    last = len(blocks) - 1 if last is None else last
    n_taps = len(taps) if n_taps is None else n_taps
    outs = (ctypes.c_void_p * max(1, n_taps))(*([tap_out] * n_taps))
    return L.ftx_vit_eval(ni._ptr(model), ni._ptr(blocks), len(blocks), ni._ptr(taps), n_taps, b, img, None, first, last, linear, attn, outs, arena,
                          arena_bytes, None)


def test_arena_bytes_answers_without_a_gpu_and_grows_with_b(ftx_lib):
    model, blocks, _ = tables()
    sizes = [ni.arena_bytes(model, len(blocks), b) for b in (1, 2, 3, 4, 8)]
    assert all(s % 256 == 0 and s > 0 for s in sizes)
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    rows = 1 * (2 + 24 * 24)
    assert sizes[0] >= 4 * rows * (10 * 768 + 2 * 3072)      # the residual stream, every block intermediate and the tap's tensor
    assert ftx_lib.ftx_vit_eval_arena_bytes(ni._ptr(model), 3, 0) == 256
    bad, _, _ = tables(dim=700)
    assert ftx_lib.ftx_vit_eval_arena_bytes(ni._ptr(bad), 3, 1) == 0 and "ftx_vit_eval_arena_bytes" in err(ftx_lib)
    with pytest.raises(RuntimeError, match="ftx_vit_eval_arena_bytes"):
        ni.arena_bytes(bad, 3, 1)


EVAL_REFUSALS = [
    ("heads", dict(heads=11), {}, "heads * 64 != dim"),
    ("dim", dict(dim=640, heads=10), {}, "dim 640"),
    ("hidden", dict(hidden=3000), {}, "hidden"),
    ("taps descending", dict(tap_blocks=(2, 0)), {}, "ascending"),
    ("taps repeated", dict(tap_blocks=(1, 1)), {}, "ascending"),
    ("tap past block_last", dict(), dict(last=1), "past block_last"),
    ("no state", dict(), dict(first=1), "holds no residual state"),
    ("block range", dict(), dict(first=2, last=1, n_taps=0), "blocks [2, 1]"),
    ("linear mode", dict(), dict(linear=2), "linear_mode"),
    ("attention mode", dict(), dict(attn=-1), "attn_mode"),
    ("no input", dict(), dict(img=None), "needs the image or tokens_in"),
    ("arena alignment", dict(), dict(arena=FAKE + 16), "256-byte aligned"),
    ("co", dict(co=98), {}, "co must be a multiple of 4"),
    ("misaligned tap output", dict(), dict(tap_out=FAKE + 4), "tap 0: stem weight, bias and output must be 16-byte aligned"),
]


@pytest.mark.parametrize("name,shape,how,text", EVAL_REFUSALS, ids=[c[0] for c in EVAL_REFUSALS])
def test_vit_eval_refuses_before_the_first_launch(ftx_lib, name, shape, how, text):
    model, blocks, taps = tables(**shape)
    assert call(ftx_lib, model, blocks, taps, **how) == EINVAL, name
    msg = err(ftx_lib)
    assert msg.startswith("ftx_vit_eval:") and text in msg, msg


def test_vit_eval_small_arena_null_parameter_and_empty_batch(ftx_lib):
    model, blocks, taps = tables()
    need = ni.arena_bytes(model, len(blocks), 2)
    assert call(ftx_lib, model, blocks, taps, b=2, arena_bytes=need - 256) == EWORKSPACE
    assert err(ftx_lib).startswith("ftx_vit_eval:") and "ftx_vit_eval_arena_bytes" in err(ftx_lib)
    blocks["fc1_w"][1] = 0
    assert call(ftx_lib, model, blocks, taps) == EINVAL and "block 1: null parameter" in err(ftx_lib)
    blocks["fc1_w"][1] = FAKE
    taps["var"][1] = 0
    assert call(ftx_lib, model, blocks, taps) == EINVAL and "tap 1: null parameter" in err(ftx_lib)
    taps["var"][1] = FAKE
    blocks["qkv_b"][2] = FAKE + 8
    assert call(ftx_lib, model, blocks, taps) == EINVAL and "block 2: parameters must be 16-byte aligned" in err(ftx_lib)
    blocks["qkv_b"][2] = FAKE
    taps["stem_w"][0] = FAKE + 4
    assert call(ftx_lib, model, blocks, taps) == EINVAL and "tap 0: stem weight" in err(ftx_lib)
    taps["stem_w"][0] = FAKE
    assert ftx_lib.ftx_vit_eval_release(FAKE) == 0 and ftx_lib.ftx_vit_eval_release(None) == 0      # nothing noted: a no-op
    assert call(ftx_lib, model, blocks, taps, b=0, arena=None, arena_bytes=0) == 0      # an empty batch is a no-op
    assert call(ftx_lib, model, blocks, taps, b=-1) == EINVAL and "batch -1" in err(ftx_lib)


PATCH_OK = dict(b=1, c=3, h=384, w=384, patch=16, dim=768, t0=2)
PATCH_REFUSALS = [
    (dict(c=1, patch=4), "multiple of 64"),          # c * patch * patch = 16
    (dict(dim=770), "dim must be a multiple of 4"),
    (dict(patch=6, h=384, w=384), "patch must be a multiple of 4"),
    (dict(h=380), "whole patches"),
    (dict(w=392 + 4), "whole patches"),
    (dict(t0=3), "t0 must be 1 or 2"),
]


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_patch_embed_refusals(ftx_lib, mode):
    fn = getattr(ftx_lib, "ftx_vit_patch_embed_" + mode)
    me = "ftx_vit_patch_embed_" + mode

    def run(ptrs=(FAKE,) * 6, tokens=FAKE, **kw):
        a = dict(PATCH_OK, **kw)
        return fn(*ptrs, a["b"], a["c"], a["h"], a["w"], a["patch"], a["dim"], a["t0"], tokens, None)
    for kw, text in PATCH_REFUSALS:
        assert run(**kw) == EINVAL, kw
        assert err(ftx_lib).startswith(me + ":") and text in err(ftx_lib), (kw, err(ftx_lib))
    assert run(ptrs=(FAKE, FAKE, FAKE + 4, FAKE, FAKE, FAKE)) == EINVAL and "16-byte aligned" in err(ftx_lib)
    assert run(tokens=None) == EINVAL and "null pointer" in err(ftx_lib)
    assert run(ptrs=(FAKE, None, FAKE, FAKE, FAKE, FAKE)) == EINVAL and "null pointer" in err(ftx_lib)
    assert run(ptrs=(FAKE, FAKE, FAKE, FAKE, None, FAKE)) == EINVAL and "dist" in err(ftx_lib)      # t0 = 2 needs dist
    assert run(ptrs=(None,) * 6, tokens=None, b=0) == 0                                              # b == 0: nothing to do
    assert run(ptrs=(None,) * 6, tokens=None, b=-1) == EINVAL


@pytest.mark.parametrize("mode", ["split", "bf16"])
def test_tap_stem_refusals(ftx_lib, mode):
    fn = getattr(ftx_lib, "ftx_vit_tap_stem_" + mode)
    me = "ftx_vit_tap_stem_" + mode

    def run(ptrs=(FAKE,) * 7, out=FAKE, b=1, g=576, t0=2, dim=768, co=96):
        return fn(*ptrs, 1e-5, b, g, t0, dim, co, out, None)
    for kw, text in ((dict(dim=700), "multiple of 64"), (dict(co=98), "co must be a multiple of 4"), (dict(t0=3), "t0"), (dict(g=0), "bad size")):
        assert run(**kw) == EINVAL, kw
        assert err(ftx_lib).startswith(me + ":") and text in err(ftx_lib), (kw, err(ftx_lib))
    assert run(ptrs=(FAKE + 8,) + (FAKE,) * 6) == EINVAL and "16-byte aligned" in err(ftx_lib)
    assert run(ptrs=(FAKE,) * 6 + (None,)) == EINVAL and "null pointer" in err(ftx_lib)
    assert run(out=None) == EINVAL and "null pointer" in err(ftx_lib)
    assert run(ptrs=(None,) * 7, out=None, b=0) == 0


def test_rows_add_bias_refusals(ftx_lib):
    f = ftx_lib.ftx_rows_add_bias
    assert f(FAKE, FAKE, FAKE, -1, 8, FAKE, None) == EINVAL and "ftx_rows_add_bias: n < 0" in err(ftx_lib)
    assert f(FAKE, FAKE, FAKE, 4, 6, FAKE, None) == EINVAL and "multiple of 4" in err(ftx_lib)
    assert f(FAKE, FAKE, None, 4, 8, FAKE, None) == EINVAL and "together" in err(ftx_lib)
    assert f(FAKE, None, FAKE, 4, 8, FAKE, None) == EINVAL and "together" in err(ftx_lib)
    assert f(None, None, None, 4, 8, FAKE, None) == EINVAL and "null pointer" in err(ftx_lib)
    assert f(FAKE + 4, None, None, 4, 8, FAKE, None) == EINVAL and "16-byte aligned" in err(ftx_lib)
    assert f(None, None, None, 0, 8, None, None) == 0


@pytest.mark.parametrize("kind,depth", [("middle", 3), ("late", 2)])
def test_emit_writes_the_modules_tensors(kind, depth):
    from fusiontransformer_amd.models.build import build_model
    cfg = small_cfg(kind, depth=depth)
    cfg.MODEL.vit_linear_impl = "ftx_split"
    if kind == "middle":
        cfg.MODEL.middle_feat_block_number = 0
    torch.manual_seed(0)
    net = build_model(cfg)[0].image_backbone
    model, blocks, taps, keep = ni.emit(net)
    bb = net.backbone
    m = model[0]
    assert (m["dim"], m["heads"], m["hidden"], m["patch"], m["grid"], m["t0"], m["in_chans"]) == (768, 12, 3072, 16, 24, 2, 3)
    assert m["eps"] == np.float32(1e-6)
    assert m["patch_w"] == bb.patch_embed.proj.weight.data_ptr() and m["patch_b"] == bb.patch_embed.proj.bias.data_ptr()
    assert m["cls"] == bb.cls_token.data_ptr() and m["dist"] == bb.dist_token.data_ptr() and m["pos"] == bb.pos_embed.data_ptr()
    assert len(blocks) == depth
    for i in range(depth):
        assert [int(blocks[i][f]) for f in ni.BLOCK_FIELDS] == [t.data_ptr() for t in ni.block_tensors(bb.blocks[i])]
    want = [0, depth - 1] if kind == "middle" else [depth - 1]
    assert [int(t["block"]) for t in taps] == want
    for t in taps:
        up = net.up[str(int(t["block"]))]
        assert [int(t[f]) for f in ("stem_w", "stem_b", "gamma", "beta", "mean", "var")] == [x.data_ptr() for x in ni.tap_tensors(up)]
        assert t["co"] == 96 and t["eps"] == np.float32(up.stem[2].eps)
    assert ni.modes(net) == (ni.LINEAR_SPLIT, ni.ATTN_FP32)
    assert len({id(t) for t in keep}) == len(keep) == 5 + 12 * depth + 6 * len(taps)


def test_modes_and_the_reason_the_switch_does_not_engage():
    from fusiontransformer_amd.models.build import build_model
    cfg = small_cfg("late")
    torch.manual_seed(0)
    net = build_model(cfg)[0].image_backbone      # vit_linear_impl = "library"
    with pytest.raises(ni.Unsupported, match="library"):
        ni.modes(net)
    net.backbone.set_linear_impl("ftx")
    with pytest.raises(ni.Unsupported, match="set_bf16"):
        ni.modes(net)
    net.backbone.set_bf16(True)
    net.backbone.set_attention_impl("ftx_bf16")
    assert ni.modes(net) == (ni.LINEAR_BF16, ni.ATTN_BF16)
    net.backbone.set_attention_impl("torch")
    with pytest.raises(ni.Unsupported, match="attn_impl"):
        ni.modes(net)
    assert net.native_eval_reason() == "the switch is off" and net.image_native_eval is False
    net.set_native_eval(True)
    img = torch.zeros(1, 3, 8, 8)
    assert net._native_executor(img) is None and net.native_eval_reason() == "training mode"
    net.eval()
    assert net._native_executor(img) is None and net.native_eval_reason() == "gradients are enabled"
    with torch.no_grad():
        assert net._native_executor(img) is None and net.native_eval_reason() == "the image is not on the GPU"
    cfg.MODEL.image_native_eval = True
    assert build_model(cfg)[0].image_backbone.image_native_eval is True
