"""Host side of the training forms of the ViT patch embedding and tap stems (include/ftx.h: ftx_vit_patch_embed_bwd_*,
ftx_vit_tap_stem_train_fwd_*, ftx_vit_tap_stem_bwd_*): a numpy restatement of the three addressings the kernels never materialise
(unfold, strip, fold), checked against torch's own unfold / fold and slicing; the new names in the header, the ctypes table and the
built library; every refusal, reached without a GPU and before anything could be launched; the switch and its reasons.

tests/test_vit_stems_train_gpu.py materialises its operands with the restatement below."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fusiontransformer_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
FAKE = 0x10000   # a 256-byte aligned address that is never dereferenced: every call below is refused on the host
EINVAL, EWORKSPACE = -1, -3
MODES = ("split", "bf16")
ENTRIES = ("ftx_vit_patch_embed_bwd_%s_workspace_bytes", "ftx_vit_patch_embed_bwd_%s", "ftx_vit_tap_stem_train_fwd_%s",
           "ftx_vit_tap_stem_bwd_%s_workspace_bytes", "ftx_vit_tap_stem_bwd_%s")


# ---------------------------------------------------------------- the three addressings, element by element
def unfold_np(img, p):
    """(b, c, h, w) -> (b gh gw, c p p): row (frame, gy, gx), column (ci, py, px) = img[frame][ci][gy p + py][gx p + px]."""
    b, c, h, w = img.shape
    gh, gw = h // p, w // p
    out = np.empty((b * gh * gw, c * p * p), dtype=img.dtype)
    for f in range(b):
        for gy in range(gh):
            for gx in range(gw):
                out[(f * gh + gy) * gw + gx] = img[f, :, gy * p:(gy + 1) * p, gx * p:(gx + 1) * p].reshape(-1)
    return out


def fold_np(rows, b, c, h, w, p):
    """The inverse permutation: rows (b gh gw, c p p) -> (b, c, h, w); every pixel takes exactly one element."""
    gh, gw = h // p, w // p
    out = np.empty((b, c, h, w), dtype=rows.dtype)
    for f in range(b):
        for gy in range(gh):
            for gx in range(gw):
                out[f, :, gy * p:(gy + 1) * p, gx * p:(gx + 1) * p] = rows[(f * gh + gy) * gw + gx].reshape(c, p, p)
    return out


def strip_np(tokens, t0):
    """(b, t0 + g, n) -> (b g, n): row r is token row (r // g) (t0 + g) + t0 + r % g."""
    b, tg, n = tokens.shape
    g = tg - t0
    flat = tokens.reshape(b * tg, n)
    return np.stack([flat[(r // g) * tg + t0 + r % g] for r in range(b * g)]) if b * g else np.empty((0, n), tokens.dtype)


def strip_store_np(rows, b, t0, g):
    """(b g, n) -> (b, t0 + g, n): rows t0.. of every frame, the t0 leading rows zero."""
    out = np.zeros((b, t0 + g, rows.shape[1]), dtype=rows.dtype)
    for r in range(b * g):
        out[r // g, t0 + r % g] = rows[r]
    return out


@pytest.mark.parametrize("b,c,gh,gw,p", [(1, 1, 2, 2, 8), (3, 3, 7, 7, 16), (2, 2, 3, 5, 4)])
def test_unfold_and_fold_are_torchs(b, c, gh, gw, p):
    img = torch.randn(b, c, gh * p, gw * p, generator=torch.Generator().manual_seed(b + c + p))
    rows = unfold_np(img.numpy(), p)
    want = F.unfold(img, kernel_size=p, stride=p).transpose(1, 2).reshape(b * gh * gw, c * p * p)
    assert np.array_equal(rows, want.numpy())
    # what PatchEmbed.forward materialises
    mine = img.reshape(b, c, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(b * gh * gw, c * p * p)
    assert np.array_equal(rows, mine.numpy())
    r = torch.randn(b * gh * gw, c * p * p, generator=torch.Generator().manual_seed(7))
    back = F.fold(r.reshape(b, gh * gw, c * p * p).transpose(1, 2), (gh * p, gw * p), kernel_size=p, stride=p)
    assert np.array_equal(fold_np(r.numpy(), b, c, gh * p, gw * p, p), back.numpy())
    assert np.array_equal(fold_np(rows, b, c, gh * p, gw * p, p), img.numpy())      # a bijection: every pixel exactly once
    # the fold is the adjoint of the unfold: autograd's gradient of the unfold is the fold of the incoming gradient
    x = img.clone().requires_grad_(True)
    F.unfold(x, kernel_size=p, stride=p).transpose(1, 2).reshape(b * gh * gw, c * p * p).backward(r)
    assert np.array_equal(fold_np(r.numpy(), b, c, gh * p, gw * p, p), x.grad.numpy())


@pytest.mark.parametrize("b,g,t0", [(1, 4, 0), (1, 4, 1), (3, 49, 2), (2, 5, 1)])
def test_strip_and_strip_store_are_slicing(b, g, t0):
    tokens = torch.randn(b, t0 + g, 8, generator=torch.Generator().manual_seed(g))
    rows = strip_np(tokens.numpy(), t0)
    assert np.array_equal(rows, tokens[:, t0:].reshape(b * g, 8).numpy())
    stored = strip_store_np(rows, b, t0, g)
    assert np.array_equal(stored[:, t0:], tokens[:, t0:].numpy()) and not stored[:, :t0].any()
    x = tokens.clone().requires_grad_(True)
    x[:, t0:].reshape(b * g, 8).backward(torch.from_numpy(rows))      # autograd's slice backward: the same zero-padded store
    assert np.array_equal(stored, x.grad.numpy())


# ---------------------------------------------------------------- the names
def test_new_entries_are_declared_bound_and_exported(ftx_lib):
    header = (ROOT / "include" / "ftx.h").read_text()
    for mode in MODES:
        for pat in ENTRIES:
            name = pat % mode
            assert re.search(r"\b%s\(" % name, header), name
            assert name in _lib.SIGNATURES, name
            assert getattr(ftx_lib, name) is not None, name
    assert "frames ascending" in header and "ftx_rows_gemm_<split|bf16>" in header      # the two orders the contract pins


def err(L):
    return L.ftx_last_error().decode()


# ---------------------------------------------------------------- refusals
PATCH_OK = dict(b=2, c=3, h=384, w=384, patch=16, dim=768, t0=2)
PATCH_REFUSALS = [(dict(b=0), "bad size"), (dict(patch=6, h=384 - 384 % 6, w=384 - 384 % 6), "patch must be a multiple of 4"),
                  (dict(c=1, patch=4, h=8, w=8), "c * patch * patch must be a multiple of 64"), (dict(dim=770), "dim must be a multiple of 4"),
                  (dict(h=380), "whole patches"), (dict(w=396), "whole patches"), (dict(t0=0), "t0 must be 1 or 2"), (dict(t0=3), "t0 must be 1 or 2")]


@pytest.mark.parametrize("mode", MODES)
def test_patch_embed_bwd_refusals(ftx_lib, mode):
    me = "ftx_vit_patch_embed_bwd_" + mode
    fn, size = getattr(ftx_lib, me), getattr(ftx_lib, me + "_workspace_bytes")
    need = size(*[PATCH_OK[k] for k in ("b", "c", "h", "w", "patch", "dim")])
    # dW is one 6 x 6 grid of tiles: min(ceil(256 / 36), 1152 / 256 = 4, 8) = 4 splits of (768, 768) partials, then ftx_colsum's own
    assert need == 4 * 4 * 768 * 768 + ftx_lib.ftx_colsum_workspace_bytes(576, 768) + (-ftx_lib.ftx_colsum_workspace_bytes(576, 768)) % 256
    assert size(0, 3, 384, 384, 16, 768) == 256 and size(2, 3, 380, 384, 16, 768) == 256

    def run(ins=(FAKE,) * 3, outs=(FAKE,) * 6, ws=FAKE, ws_bytes=need, **kw):
        a = dict(PATCH_OK, **kw)
        return fn(*ins, a["b"], a["c"], a["h"], a["w"], a["patch"], a["dim"], a["t0"], *outs, ws, ws_bytes, None)
    for kw, text in PATCH_REFUSALS:
        assert run(**kw) == EINVAL, kw
        assert err(ftx_lib).startswith(me + ":") and text in err(ftx_lib), (kw, err(ftx_lib))
    for i in range(3):      # dtokens, img, W
        assert run(ins=tuple(FAKE + 4 * (j == i) for j in range(3))) == EINVAL and "16-byte aligned" in err(ftx_lib), i
    for i in range(6):      # dW, dbias, dcls, ddist, dpos, dimg
        assert run(outs=tuple(FAKE + 8 * (j == i) for j in range(6))) == EINVAL and "16-byte aligned" in err(ftx_lib), i
    assert run(ws=FAKE + 4) == EINVAL and "16-byte aligned" in err(ftx_lib)
    assert run(ins=(None, FAKE, FAKE)) == EINVAL and "null pointer" in err(ftx_lib)
    assert run(ins=(FAKE, None, FAKE)) == EINVAL and "null pointer" in err(ftx_lib)
    assert run(ins=(FAKE, FAKE, None)) == EINVAL and "W with dimg" in err(ftx_lib)
    assert run(outs=(None,) + (FAKE,) * 5) == EINVAL and "null pointer" in err(ftx_lib)
    assert run(outs=(FAKE, FAKE, FAKE, None, FAKE, FAKE)) == EINVAL and "ddist" in err(ftx_lib)      # t0 = 2 needs ddist
    assert run(ws=None) == EINVAL and "null pointer" in err(ftx_lib)
    assert run(dim=772) == EINVAL and "multiple of 64 for the image gradient" in err(ftx_lib)          # only with dimg
    assert run(ws_bytes=need - 1) == EWORKSPACE and "workspace %d < required %d" % (need - 1, need) in err(ftx_lib)
    assert run(ws_bytes=0) == EWORKSPACE


@pytest.mark.parametrize("mode", MODES)
def test_tap_stem_train_refusals(ftx_lib, mode):
    fwd_name, bwd_name = "ftx_vit_tap_stem_train_fwd_" + mode, "ftx_vit_tap_stem_bwd_" + mode
    fwd, bwd, size = getattr(ftx_lib, fwd_name), getattr(ftx_lib, bwd_name), getattr(ftx_lib, bwd_name + "_workspace_bytes")
    need = size(2, 576, 768, 96)
    # the masked gradient, the product of the rows GEMM, four partials (96 x 768 is 6 tiles: min(43, 1152 / 256, 8) = 4 splits), ftx_colsum
    colsum = ftx_lib.ftx_colsum_workspace_bytes(1152, 96)
    assert need == 4 * 1152 * 96 + 4 * 1152 * 768 + 4 * 4 * 96 * 768 + colsum + (-colsum) % 256
    assert size(0, 576, 768, 96) == 256

    def f(ptrs=(FAKE,) * 3, rows=FAKE, b=1, g=576, t0=2, dim=768, co=96):
        return fwd(*ptrs, b, g, t0, dim, co, rows, None)

    def r(ins=(FAKE,) * 4, outs=(FAKE,) * 3, ws=FAKE, ws_bytes=need, b=2, g=576, t0=2, dim=768, co=96):
        return bwd(*ins, b, g, t0, dim, co, *outs, ws, ws_bytes, None)
    refusals = ((dict(dim=700), "multiple of 64"), (dict(co=98), "co must be a multiple of 4"), (dict(t0=3), "t0 must be 0, 1 or 2"),
                (dict(t0=-1), "t0 must be 0, 1 or 2"), (dict(g=0), "bad size"), (dict(dim=32), "bad size"))
    for run, me in ((f, fwd_name), (r, bwd_name)):
        for kw, text in refusals:
            assert run(**kw) == EINVAL, (me, kw)
            assert err(ftx_lib).startswith(me + ":") and text in err(ftx_lib), (me, kw, err(ftx_lib))
    for i in range(3):
        assert f(ptrs=tuple(FAKE + 8 * (j == i) for j in range(3))) == EINVAL and "16-byte aligned" in err(ftx_lib)
        assert f(ptrs=tuple(None if j == i else FAKE for j in range(3))) == EINVAL and "null pointer" in err(ftx_lib)
    assert f(rows=FAKE + 4) == EINVAL and "16-byte aligned" in err(ftx_lib)
    assert f(rows=None) == EINVAL and "null pointer" in err(ftx_lib)
    assert f(ptrs=(None,) * 3, rows=None, b=0) == 0 and f(b=-1) == EINVAL
    for i in range(4):
        assert r(ins=tuple(FAKE + 4 * (j == i) for j in range(4))) == EINVAL and "16-byte aligned" in err(ftx_lib)
        assert r(ins=tuple(None if j == i else FAKE for j in range(4))) == EINVAL and "null pointer" in err(ftx_lib)
    for i in range(3):
        assert r(outs=tuple(FAKE + 4 * (j == i) for j in range(3))) == EINVAL and "16-byte aligned" in err(ftx_lib)
        assert r(outs=tuple(None if j == i else FAKE for j in range(3))) == EINVAL and "null pointer" in err(ftx_lib)
    assert r(ws=FAKE + 8) == EINVAL and r(ws=None) == EINVAL and r(b=0) == EINVAL
    assert r(ws_bytes=need - 1) == EWORKSPACE and "workspace %d < required %d" % (need - 1, need) in err(ftx_lib)


def test_functional_nodes_refuse_bad_operands_before_a_launch(monkeypatch):
    """ValueError from the wrappers' own checks; under tests/nolaunch.py a launch would be an AssertionError."""
    from fusiontransformer_amd import functional as spf
    from tests.nolaunch import NoLaunch
    monkeypatch.setattr(_lib, "load", lambda: NoLaunch())
    img, w = torch.zeros(1, 3, 32, 32), torch.zeros(64, 3, 16, 16)
    vec, pos = torch.zeros(64), torch.zeros(6, 64)
    with pytest.raises(ValueError, match="mode must be"):
        spf.vit_patch_embed(img, w, vec, vec, vec, pos, mode="fp32")
    with pytest.raises(ValueError, match="CUDA"):
        spf.vit_patch_embed(img, w, vec, vec, vec, pos)
    with pytest.raises(ValueError, match="mode must be"):
        spf.vit_tap_stem(torch.zeros(1, 6, 64), torch.zeros(8, 64), torch.zeros(8), 2, mode="library")
    with pytest.raises(ValueError, match="CUDA"):
        spf.vit_tap_stem(torch.zeros(1, 6, 64), torch.zeros(8, 64), torch.zeros(8), 2)
    assert not spf.vit_patch_embed_supported(img, w)


# ---------------------------------------------------------------- the switch
def test_the_switch_is_read_with_the_others_and_says_why_it_does_not_engage():
    from fusiontransformer_amd.models.build import build_image_model, build_model
    from tests.helpers import small_cfg
    cfg = small_cfg("late")
    torch.manual_seed(0)
    net = build_model(cfg)[0].image_backbone
    bb = net.backbone
    assert bb.image_native_stems is False and net.native_stems_reason() == "the switch is off"
    img = torch.zeros(1, 3, 384, 384)
    assert bb.native_stems_mode(img) is None and net.native_stems_reason() == "the switch is off"
    assert net.set_native_stems(True) is net and bb.image_native_stems is True
    bb.eval()
    assert bb.native_stems_mode(img) is None and net.native_stems_reason() == "eval mode"
    bb.train()
    with torch.no_grad():
        assert bb.native_stems_mode(img) is None and net.native_stems_reason() == "gradients are disabled"
    assert bb.native_stems_mode(img) is None and net.native_stems_reason() == "the input is not a float32 tensor on the GPU"
    # the switch is independent of image_native_train, and off again leaves no state
    assert bb.image_native_train is False
    net.set_native_stems(False)
    assert bb.image_native_stems is False and net.native_stems_reason() == "the switch is off"
    cfg.MODEL.image_native_stems = True
    assert build_model(cfg)[0].image_backbone.backbone.image_native_stems is True
    stn = small_cfg("late")
    stn.MODEL.TYPE, stn.MODEL.USE_FUSION, stn.MODEL.USE_LIDAR = "ImageSeg", False, False
    assert build_image_model(stn)[0].image_backbone.backbone.image_native_stems is False
    stn.MODEL.image_native_stems = True
    seg = build_image_model(stn)[0].image_backbone
    assert seg.backbone.image_native_stems is True and seg.native_stems_reason() == "the switch is off"
    # on the CPU the forward is the existing one: full_tokens only widens the view
    t = torch.zeros(1, bb.num_tokens + 4, 8)
    assert bb._tap_view(t).shape[1] == 4 and bb._tap_view(t, True) is t
