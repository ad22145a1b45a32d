"""bf16-operand attention without a GPU: the C entry points exist and refuse bad arguments before anything is launched, and the
model layer carries attn_impl="ftx_bf16" to every block and into the trunk's graph keys."""
import ctypes
import re

import torch

from fusiontransformer_amd import _lib
from tests.test_cabi import ROOT, declared_symbols

FAKE = ctypes.c_void_p(4096)   # never dereferenced: every call below must fail its argument check first


def test_bf16_entries_are_exported_and_declared(ftx_lib):
    for name in ("ftx_attn_fwd_bf16", "ftx_attn_bwd_bf16"):
        assert name in declared_symbols(), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(ftx_lib, name), name
    header = open(f"{ROOT}/include/ftx.h").read()
    assert re.search(r"round-to-nearest-even", header), "the precision contract is stated in the header"


def test_bf16_fwd_refuses_bad_arguments(ftx_lib):
    L = ftx_lib
    assert L.ftx_attn_fwd_bf16(FAKE, 1, 578, 12, 32, 0.125, FAKE, FAKE, 0, 0, None) == -1
    assert b"head dim must be 64" in L.ftx_last_error()
    assert L.ftx_attn_fwd_bf16(FAKE, 1, 578, 12, 64, 0.125, FAKE, FAKE, 3, 2, None) == -1
    assert b"not a built tiling" in L.ftx_last_error()
    assert L.ftx_attn_fwd_bf16(None, 1, 578, 12, 64, 0.125, FAKE, FAKE, 0, 0, None) == -1
    assert b"null pointer" in L.ftx_last_error()


def test_bf16_bwd_refuses_bad_arguments(ftx_lib):
    L = ftx_lib
    ws = L.ftx_attn_bwd_workspace_bytes(2, 578, 12)
    assert L.ftx_attn_bwd_bf16(FAKE, FAKE, FAKE, FAKE, 2, 578, 12, 32, 0.125, FAKE, FAKE, ws, 0, 0, None) == -1
    assert b"head dim must be 64" in L.ftx_last_error()
    assert L.ftx_attn_bwd_bf16(FAKE, FAKE, FAKE, FAKE, 2, 578, 12, 64, 0.125, FAKE, FAKE, ws, 1, 3, None) == -1
    assert b"not a built tiling" in L.ftx_last_error()
    assert L.ftx_attn_bwd_bf16(FAKE, FAKE, FAKE, FAKE, 2, 578, 12, 64, 0.125, FAKE, FAKE, ws - 4, 0, 0, None) == -3
    assert b"workspace" in L.ftx_last_error()
    assert L.ftx_attn_bwd_bf16(FAKE, FAKE, FAKE, FAKE, 2, 578, 12, 64, 0.125, FAKE, None, ws, 0, 0, None) == -1
    assert b"null pointer" in L.ftx_last_error()


def _trunk(attn_impl):
    from fusiontransformer_amd.models.build import build_model
    from tests.helpers import small_cfg
    cfg = small_cfg("middle")
    cfg.MODEL.attn_impl = attn_impl
    torch.manual_seed(0)
    model, _, _ = build_model(cfg)
    return model.image_backbone.backbone


def test_model_keeps_ftx_bf16_on_every_block():
    vit = _trunk("ftx_bf16")
    assert len(vit.blocks) == 2
    assert all(blk.attn.attn_impl == "ftx_bf16" for blk in vit.blocks)
    assert not any(getattr(blk.attn.qkv, "ftx_bf16", False) for blk in vit.blocks), "attn_impl does not switch the GEMMs to bf16"


def test_graph_key_distinguishes_bf16_attention(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)   # the key records the device; no GPU is touched here
    a, b = _trunk("ftx"), _trunk("ftx_bf16")
    assert a.graph_taps and b.graph_taps
    x = torch.zeros(1, 3, 384, 384)
    assert a._graph_key(x) != b._graph_key(x)
    b.set_attention_impl("ftx")
    assert a._graph_key(x) == b._graph_key(x)

