"""bf16-operand ViT Linears without a GPU: the C entry points exist, refuse bad arguments before anything is launched and report the
tile / split table; the model layer carries vit_linear_impl to every Linear and into both graph keys."""
import ctypes
import re

import pytest
import torch

from fusiontransformer_amd import _lib
from tests.test_cabi import ROOT, declared_symbols

FAKE = ctypes.c_void_p(4096)      # never dereferenced: every call below must fail its argument check first
ODD = ctypes.c_void_p(4096 + 4)   # not 16-byte aligned
ENTRIES = ("ftx_dense_gemm_bf16", "ftx_dense_wgrad_bf16", "ftx_dense_wgrad_bf16_workspace_bytes", "ftx_dense_bf16_tile")


def test_dense_entries_are_exported_and_declared(ftx_lib):
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(ftx_lib, name), name
    header = open(f"{ROOT}/include/ftx.h").read()
    block = header[header.index("bf16-operand ViT Linears"):]
    assert re.search(r"round-to-nearest-even", block[:2000]), "the precision contract is stated next to the entries"
    for epi, v in (("NONE", 0), ("BIAS", 1), ("BIAS_GELU", 2), ("DGELU", 3)):
        assert re.search(rf"#define FTX_EPI_{epi} {v}\b", header), epi


def _gemm(L, a=FAKE, w=FAKE, w_kn=0, bias=FAKE, pre_in=FAKE, m=578, n=768, k=768, epi=1, out=FAKE, pre_out=FAKE):
    return L.ftx_dense_gemm_bf16(a, w, w_kn, bias, pre_in, m, n, k, epi, out, pre_out, None)


def test_gemm_refuses_bad_arguments(ftx_lib):
    L = ftx_lib
    cases = [
        (dict(m=-1), b"bad size"),
        (dict(k=32), b"bad size"),
        (dict(k=96), b"multiple of 64"),
        (dict(n=770), b"multiple of 4"),
        (dict(w_kn=2), b"w_kn"),
        (dict(epi=4), b"unknown epilogue"),
        (dict(a=None), b"null pointer"),
        (dict(out=None), b"null pointer"),
        (dict(epi=1, bias=None), b"null pointer (bias)"),
        (dict(epi=2, bias=None), b"null pointer (bias)"),
        (dict(epi=2, pre_out=None), b"null pointer (pre_out)"),
        (dict(epi=3, pre_in=None), b"null pointer (pre_in)"),
        (dict(a=ODD), b"16-byte aligned"),
        (dict(epi=3, pre_in=ODD), b"16-byte aligned"),
    ]
    for kw, msg in cases:
        assert _gemm(L, **kw) == -1, kw
        assert msg in L.ftx_last_error(), (kw, L.ftx_last_error())
    # m == 0: nothing to do, nothing launched, even with null operands
    assert _gemm(L, a=None, w=None, out=None, m=0) == 0


def test_wgrad_refuses_bad_arguments(ftx_lib):
    L = ftx_lib
    m, n, k = 2312, 768, 768
    ws = L.ftx_dense_wgrad_bf16_workspace_bytes(m, n, k)
    assert ws == 8 * n * k * 4, "proj at batch 4 splits its rows 8 ways"
    assert L.ftx_dense_wgrad_bf16(FAKE, FAKE, m, 770, k, FAKE, FAKE, ws, None) == -1
    assert b"multiples of 4" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_bf16(FAKE, FAKE, -1, n, k, FAKE, FAKE, ws, None) == -1
    assert b"bad size" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_bf16(FAKE, FAKE, m, n, k, None, FAKE, ws, None) == -1
    assert b"null pointer (dW)" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_bf16(None, FAKE, m, n, k, FAKE, FAKE, ws, None) == -1
    assert b"null pointer" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_bf16(FAKE, ODD, m, n, k, FAKE, FAKE, ws, None) == -1
    assert b"16-byte aligned" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_bf16(FAKE, FAKE, m, n, k, FAKE, FAKE, ws - 4, None) == -3
    assert b"workspace" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_bf16(FAKE, FAKE, m, n, k, FAKE, None, ws, None) == -3
    # an unsplit shape needs no workspace at all
    assert L.ftx_dense_wgrad_bf16_workspace_bytes(33, n, k) == 256


# (M, linear) -> forward tile, dX tile, weight-gradient splits.  K, N of each Linear as nn.Linear(K, N); M = 578 tokens x batch.
LINEARS = {"qkv": (768, 2304), "proj": (768, 768), "fc1": (768, 3072), "fc2": (3072, 768)}
TILES = {
    1: {"qkv": ((64, 64), (64, 64), 1), "proj": ((64, 64), (64, 64), 1), "fc1": ((64, 64), (64, 64), 1), "fc2": ((64, 64), (64, 64), 1)},
    33: {"qkv": ((64, 64), (64, 64), 1), "proj": ((64, 64), (64, 64), 1), "fc1": ((64, 64), (64, 64), 1), "fc2": ((64, 64), (64, 64), 1)},
    578: {"qkv": ((64, 64), (64, 64), 2), "proj": ((64, 64), (64, 64), 2), "fc1": ((64, 64), (64, 64), 2), "fc2": ((64, 64), (64, 64), 2)},
    2312: {"qkv": ((128, 128), (64, 64), 3), "proj": ((64, 64), (64, 64), 8), "fc1": ((128, 128), (64, 64), 2), "fc2": ((64, 64), (128, 128), 2)},
    2313: {"qkv": ((128, 128), (64, 64), 3), "proj": ((64, 64), (64, 64), 8), "fc1": ((128, 128), (64, 64), 2), "fc2": ((64, 64), (128, 128), 2)},
    4624: {"qkv": ((128, 128), (64, 128), 3), "proj": ((64, 128), (64, 128), 8), "fc1": ((128, 128), (64, 128), 2), "fc2": ((64, 128), (128, 128), 2)},
}


@pytest.mark.parametrize("m", sorted(TILES))
def test_tile_query_matches_the_table(ftx_lib, m):
    from fusiontransformer_amd import functional as spf
    for name, (k, n) in LINEARS.items():
        fwd, dx, splits = TILES[m][name]
        assert spf.dense_bf16_tile(0, m, n, k) == fwd + (1,), (m, name, "forward")
        assert spf.dense_bf16_tile(0, m, k, n) == dx + (1,), (m, name, "dX")
        assert spf.dense_bf16_tile(1, m, n, k) == (128, 128, splits), (m, name, "dW")
        ws = ftx_lib.ftx_dense_wgrad_bf16_workspace_bytes(m, n, k)
        assert ws == (splits * n * k * 4 if splits > 1 else 256), (m, name)


def test_tile_query_refuses_bad_arguments(ftx_lib):
    a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert ftx_lib.ftx_dense_bf16_tile(2, 578, 768, 768, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1
    assert b"form" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_dense_bf16_tile(0, 0, 768, 768, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1
    assert b"bad size" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_dense_bf16_tile(0, 578, 768, 768, None, ctypes.byref(b), ctypes.byref(c)) == -1
    assert b"null pointer" in ftx_lib.ftx_last_error()


# ---------------------------------------------------------------- model layer
def _lins(vit):
    return [lin for blk in vit.blocks for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2)]


def _trunk(**model_kw):
    from fusiontransformer_amd.models.build import build_model
    from tests.helpers import small_cfg
    cfg = small_cfg("middle")
    for k, v in model_kw.items():
        cfg.MODEL[k] = v
    torch.manual_seed(0)
    model, _, _ = build_model(cfg)
    return model.image_backbone.backbone


def test_linear_impl_defaults_to_library():
    vit = _trunk()
    assert all(lin.ftx_linear_impl == "library" for lin in _lins(vit))


def test_linear_impl_reaches_every_linear():
    vit = _trunk(vit_linear_impl="ftx")
    assert len(vit.blocks) == 2
    assert all(lin.ftx_linear_impl == "ftx" for lin in _lins(vit))
    assert not any(getattr(lin, "ftx_bf16", False) for lin in _lins(vit)), "the impl does not switch precision"


def test_linear_impl_default_ignores_the_environment(monkeypatch):
    """Only cfg.MODEL.vit_linear_impl chooses: FTX_VIT_LINEAR (a switch since removed) left in the environment changes nothing."""
    monkeypatch.setenv("FTX_VIT_LINEAR", "ftx")
    vit = _trunk()
    assert len(vit.blocks) == 2
    assert all(lin.ftx_linear_impl == "library" for lin in _lins(vit))
    assert not any(getattr(lin, "ftx_bf16", False) for lin in _lins(vit)), "the impl does not switch precision"


def test_linear_impl_kwarg_and_method():
    from fusiontransformer_amd.models.image_models_billinear import Net2DBillinear
    net = Net2DBillinear(num_classes=4, dual_head=True, backbone_2d_kwargs=dict(vit_depth=2, vit_linear_impl="ftx", late_feat_block_number=1))
    assert all(lin.ftx_linear_impl == "ftx" for lin in _lins(net.backbone))
    net.backbone.set_linear_impl("library")
    assert all(lin.ftx_linear_impl == "library" for lin in _lins(net.backbone))
    with pytest.raises(ValueError):
        net.backbone.set_linear_impl("triton")


class _Cuda(torch.Tensor):
    """A CPU tensor that reports is_cuda, to drive the routing predicates without a GPU."""

    @property
    def is_cuda(self):
        return True


def test_linear_impl_is_inert_without_bf16(monkeypatch):
    """set_bf16(False): the ftx setting routes nothing to the new kernels; set_bf16(True) turns the fused MLP route on."""
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.models import transformers as T
    b = _trunk(vit_linear_impl="ftx")
    xc = torch.zeros(1, 5, 768).as_subclass(_Cuda)
    mlp = b.blocks[0].mlp
    assert not mlp._fused_ftx(xc)
    routed = []
    monkeypatch.setattr(spf, "vit_linear", lambda *a, **k: routed.append("ftx"))
    monkeypatch.setattr(T._LinearFn, "apply", staticmethod(lambda *a: routed.append(("library", a[3]))))
    T._linear(xc, b.blocks[0].attn.qkv)
    assert routed == [("library", False)]
    b.set_bf16(True)
    assert mlp._fused_ftx(xc)
    T._linear(xc, b.blocks[0].attn.qkv)
    assert routed[-1] == "ftx"
    b.set_linear_impl("library")
    T._linear(xc, b.blocks[0].attn.qkv)
    assert routed[-1] == ("library", True) and not mlp._fused_ftx(xc)
    b.set_linear_impl("ftx")
    mlp.act = torch.nn.GELU(approximate="tanh")
    assert not mlp._fused_ftx(xc), "only the exact-erf GELU is fused"
    b.set_bf16(False)
    mlp.act = torch.nn.GELU()
    assert not mlp._fused_ftx(xc)


def test_graph_keys_distinguish_linear_impl(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)   # the key records the device; no GPU is touched here
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    a, b = _trunk(), _trunk(vit_linear_impl="ftx")
    for t in (a, b):
        t.set_bf16(True)
    assert a.graph_taps and b.graph_taps
    x = torch.zeros(1, 3, 384, 384)
    assert a._graph_key(x) != b._graph_key(x)
    b.set_linear_impl("library")
    assert a._graph_key(x) == b._graph_key(x)

    # the forward-only graph's key: record what _inference_graph looks up instead of capturing
    from fusiontransformer_amd.models.transformers import Image2DTransformer
    monkeypatch.setattr(Image2DTransformer, "_capture_inference", lambda self, inp: None)
    xc = x.as_subclass(_Cuda)
    b.eval()
    keys = []
    for impl in ("library", "ftx"):
        b.set_linear_impl(impl)
        with torch.no_grad():
            b._inference_graph(xc)
        keys.append(set(b._infer_cache))
    assert len(keys[0]) == 1 and len(keys[1]) == 2, "switching the impl selects another forward-only graph"
