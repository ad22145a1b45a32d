"""fp32-accurate ViT Linears on the bf16 MFMA (three-piece operand split, vit_linear_impl="ftx_split") without a GPU: the C entry
points exist, state their contract, refuse bad arguments before anything is launched and report the tile / split table; the model layer
carries the impl to every Linear, routes on it with bf16 off and on, and into both graph keys; and tests/split_ref.py's emulation
reconstructs every float exactly and shows that gate G2 of tests/test_vit_linear_split_gpu.py tells six products from fewer."""
import ctypes
import re

import pytest
import torch

from fusiontransformer_amd import _lib
from tests import split_ref as R
from tests.test_cabi import ROOT, declared_symbols

FAKE = ctypes.c_void_p(4096)      # never dereferenced: every call below must fail its argument check first
ODD = ctypes.c_void_p(4096 + 4)   # not 16-byte aligned
ENTRIES = ("ftx_dense_gemm_split", "ftx_dense_wgrad_split", "ftx_dense_wgrad_split_workspace_bytes", "ftx_dense_split_tile")


def test_split_entries_are_exported_and_declared(ftx_lib):
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(ftx_lib, name), name
    header = open(f"{ROOT}/include/ftx.h").read()
    block = header[header.index("three-piece operand split"):]
    block = block[:block.index("int ftx_dense_split_tile")]
    assert len(block) < 4000, "the contract sits next to the entries"
    for text in (r"h = bf16\(x\)", r"m = bf16\(x - h\)", r"l = bf16\(\(x - h\) - m\)", r"round-to-nearest-even", r"2\^127", r"2\^-126",
                 r"hh, hm, mh, hl, lh, mm", r"2\.01 \* 2\^-24", r"v_mfma_f32_32x32x16_bf16", r"No atomics", r"m = l = 0"):
        assert re.search(text, block), text
    for name in ENTRIES:
        assert name in header[header.index("three-piece operand split"):], name


def _gemm(L, a=FAKE, w=FAKE, w_kn=0, bias=FAKE, pre_in=FAKE, m=578, n=768, k=768, epi=1, out=FAKE, pre_out=FAKE):
    return L.ftx_dense_gemm_split(a, w, w_kn, bias, pre_in, m, n, k, epi, out, pre_out, None)


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
        assert b"ftx_dense_gemm_split" in L.ftx_last_error()
    # m == 0: nothing to do, nothing launched, even with null operands
    assert _gemm(L, a=None, w=None, out=None, m=0) == 0


def test_wgrad_refuses_bad_arguments(ftx_lib):
    L = ftx_lib
    m, n, k = 2312, 768, 768
    ws = L.ftx_dense_wgrad_split_workspace_bytes(m, n, k)
    assert ws == 8 * n * k * 4, "proj at batch 4 splits its rows 8 ways"
    assert L.ftx_dense_wgrad_split(FAKE, FAKE, m, 770, k, FAKE, FAKE, ws, None) == -1
    assert b"multiples of 4" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_split(FAKE, FAKE, -1, n, k, FAKE, FAKE, ws, None) == -1
    assert b"bad size" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_split(FAKE, FAKE, m, n, k, None, FAKE, ws, None) == -1
    assert b"null pointer (dW)" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_split(None, FAKE, m, n, k, FAKE, FAKE, ws, None) == -1
    assert b"null pointer" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_split(FAKE, ODD, m, n, k, FAKE, FAKE, ws, None) == -1
    assert b"16-byte aligned" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_split(FAKE, FAKE, m, n, k, FAKE, FAKE, ws - 4, None) == -3
    assert b"workspace" in L.ftx_last_error()
    assert L.ftx_dense_wgrad_split(FAKE, FAKE, m, n, k, FAKE, None, ws, None) == -3
    # an unsplit shape needs no workspace at all
    assert L.ftx_dense_wgrad_split_workspace_bytes(33, n, k) == 256


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
        assert spf.dense_split_tile(0, m, n, k) == fwd + (1,), (m, name, "forward")
        assert spf.dense_split_tile(0, m, k, n) == dx + (1,), (m, name, "dX")
        assert spf.dense_split_tile(1, m, n, k) == (128, 128, splits), (m, name, "dW")
        ws = ftx_lib.ftx_dense_wgrad_split_workspace_bytes(m, n, k)
        assert ws == (splits * n * k * 4 if splits > 1 else 256), (m, name)


def test_tile_query_refuses_bad_arguments(ftx_lib):
    a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert ftx_lib.ftx_dense_split_tile(2, 578, 768, 768, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1
    assert b"form" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_dense_split_tile(0, 0, 768, 768, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1
    assert b"bad size" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_dense_split_tile(0, 578, 768, 768, None, ctypes.byref(b), ctypes.byref(c)) == -1
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


def test_split_impl_reaches_every_linear_and_default_stays_library():
    assert all(lin.ftx_linear_impl == "library" for lin in _lins(_trunk()))
    vit = _trunk(vit_linear_impl="ftx_split")
    assert len(vit.blocks) == 2
    assert all(lin.ftx_linear_impl == "ftx_split" for lin in _lins(vit))
    assert not any(getattr(lin, "ftx_bf16", False) for lin in _lins(vit)), "the impl does not switch precision"


def test_split_impl_kwarg_and_method():
    from fusiontransformer_amd.models.image_models_billinear import Net2DBillinear
    net = Net2DBillinear(num_classes=4, dual_head=True, backbone_2d_kwargs=dict(vit_depth=2, vit_linear_impl="ftx_split", late_feat_block_number=1))
    assert all(lin.ftx_linear_impl == "ftx_split" for lin in _lins(net.backbone))
    net.backbone.set_linear_impl("library")
    assert all(lin.ftx_linear_impl == "library" for lin in _lins(net.backbone))
    net.backbone.set_linear_impl("ftx_split")
    assert all(lin.ftx_linear_impl == "ftx_split" for lin in _lins(net.backbone))
    with pytest.raises(ValueError):
        net.backbone.set_linear_impl("ftx_split3")


class _Cuda(torch.Tensor):
    """A CPU tensor that reports is_cuda, to drive the routing predicates without a GPU."""

    @property
    def is_cuda(self):
        return True


def test_split_routes_with_bf16_off_and_on_and_ftx_stays_inert(monkeypatch):
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.models import transformers as T
    b = _trunk(vit_linear_impl="ftx_split")
    xc = torch.zeros(1, 5, 768).as_subclass(_Cuda)
    mlp, qkv = b.blocks[0].mlp, b.blocks[0].attn.qkv
    routed = []
    monkeypatch.setattr(spf, "vit_linear", lambda *a, **k: routed.append(("vit_linear", k.get("mode", "bf16"))))
    monkeypatch.setattr(spf, "vit_mlp", lambda *a, **k: routed.append(("vit_mlp", k.get("mode", "bf16"))))
    monkeypatch.setattr(T._LinearFn, "apply", staticmethod(lambda *a: routed.append(("library", a[3]))))
    for on in (False, True):
        b.set_bf16(on)
        assert mlp._fused_ftx(xc), on
        T._linear(xc, qkv)
        assert routed[-1] == ("vit_linear", "split"), (on, routed)
        mlp(xc)
        assert routed[-1] == ("vit_mlp", "split"), (on, routed)
    # "ftx" keeps its meaning: inert while set_bf16 is off, the bf16 kernels while it is on
    b.set_linear_impl("ftx")
    b.set_bf16(False)
    assert not mlp._fused_ftx(xc)
    T._linear(xc, qkv)
    assert routed[-1] == ("library", False)
    b.set_bf16(True)
    assert mlp._fused_ftx(xc)
    T._linear(xc, qkv)
    assert routed[-1] == ("vit_linear", "bf16")
    mlp(xc)
    assert routed[-1] == ("vit_mlp", "bf16")
    # the library impl never reaches the kernels
    b.set_linear_impl("library")
    for on in (False, True):
        b.set_bf16(on)
        assert not mlp._fused_ftx(xc)
        T._linear(xc, qkv)
        assert routed[-1] == ("library", on)
    # only the exact-erf GELU is fused, in split mode too
    b.set_linear_impl("ftx_split")
    mlp.act = torch.nn.GELU(approximate="tanh")
    assert not mlp._fused_ftx(xc)


def test_split_mode_falls_back_to_the_fp32_library_path_on_the_cpu():
    """A call vit_linear_supported refuses (here: CPU tensors) runs _LinearFn(..., False): fp32, not the bf16 library path."""
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.models.transformers import _LinearFn
    torch.manual_seed(3)
    x, w, b = torch.randn(5, 64), torch.randn(128, 64), torch.randn(128)
    assert torch.equal(spf.vit_linear(x, w, b, mode="split"), _LinearFn.apply(x, w, b, False))
    assert not torch.equal(spf.vit_linear(x, w, b, mode="split"), _LinearFn.apply(x, w, b, True))
    w2, b2 = torch.randn(64, 128), torch.randn(64)
    ref = _LinearFn.apply(torch.nn.functional.gelu(_LinearFn.apply(x, w, b, False)), w2, b2, False)
    assert torch.equal(spf.vit_mlp(x, w, b, w2, b2, mode="split"), ref)
    with pytest.raises(ValueError):
        spf.vit_linear(x, w, b, mode="fp8")


def test_graph_keys_distinguish_the_three_impls(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)   # the key records the device; no GPU is touched here
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    trunks = {impl: _trunk(vit_linear_impl=impl) for impl in ("library", "ftx", "ftx_split")}
    x = torch.zeros(1, 3, 384, 384)
    for on in (False, True):
        keys = {}
        for impl, t in trunks.items():
            t.set_bf16(on)
            assert t.graph_taps
            keys[impl] = t._graph_key(x)
        assert len(set(keys.values())) == 3, on
        assert all([impl for impl, _ in blk[1]] == ["ftx_split"] * 4 for blk in keys["ftx_split"][6])
    trunks["ftx_split"].set_linear_impl("library")
    assert trunks["ftx_split"]._graph_key(x) == trunks["library"]._graph_key(x)

    # the forward-only graph's key: record what _inference_graph looks up instead of capturing
    from fusiontransformer_amd.models.transformers import Image2DTransformer
    monkeypatch.setattr(Image2DTransformer, "_capture_inference", lambda self, inp: None)
    xc = x.as_subclass(_Cuda)
    b = trunks["ftx"]
    b.eval()
    sizes = []
    for impl in ("library", "ftx", "ftx_split"):
        b.set_linear_impl(impl)
        with torch.no_grad():
            b._inference_graph(xc)
        sizes.append(len(b._infer_cache))
    assert sizes == [1, 2, 3], "switching the impl selects another forward-only graph"


# ---------------------------------------------------------------- the emulation: exact pieces, and a gate that tells
def test_pieces_reconstruct_every_float_exactly():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1 << 20, generator=g) * torch.exp2(torch.randint(-60, 61, (1 << 20,), generator=g).float())
    big = torch.tensor(2.0 ** 127).float() * (1 - 2.0 ** -24)   # the largest float below 2^127
    edge = torch.tensor([0.0, -0.0, 1.0, -2.0, 2.0 ** -20, 2.0 ** 100, float(big), -float(big), 2.0 ** -126, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24,
                         3.0 * 2.0 ** -126], dtype=torch.float32)
    assert float(big) < 2.0 ** 127 and float(torch.nextafter(big, torch.tensor(float("inf")))) == 2.0 ** 127
    for t in (x, edge):
        h, m, l = R.split3(t)
        for p in (h, m, l):
            assert torch.equal(p, p.to(torch.bfloat16).float()), "every piece is a bf16 number"
        s = (h + m) + l   # exact in fp32: h + m has at most 16 significant bits and h + m + l is x itself
        assert torch.equal(s.view(torch.int32), t.view(torch.int32)) or torch.equal(s, t), "h + m + l == x bit for bit"
        assert torch.equal(h.double() + m.double() + l.double(), t.double())
    assert torch.equal(torch.signbit(R.split3(edge[:2])[0]), torch.tensor([False, True])), "the sign of zero stays on h"
    # inf and NaN stay on h alone
    h, m, l = R.split3(torch.tensor([float("inf"), -float("inf"), float("nan"), 3.4e38]))
    assert torch.isinf(h[:2]).all() and torch.isnan(h[2]) and torch.isinf(h[3]), "above 2^127 h rounds to inf (the stated range)"
    assert torch.equal(m, torch.zeros(4)) and torch.equal(l, torch.zeros(4))


@pytest.mark.parametrize("k", [768, 3072])
def test_g2_passes_six_products_and_fails_five_and_three(k):
    """Gate G2 (E <= T / 2) on the CPU emulation with fp32 accumulation in k-chunks of 16: the six-product scheme passes in both
    accumulator forms, five (mm dropped) and three (hh, hm, mh) products fail however they accumulate, and so does plain bf16."""
    g = torch.Generator().manual_seed(k)
    a = torch.randn(96, k, generator=g)
    b = (torch.randn(80, k, generator=g) * 0.02).t().contiguous()
    figures = {}
    for two in (True, False):
        out = R.gemm(a, b, R.SIX, accumulate="fp32", two_accumulators=two)
        figures[("six", two)] = R.g2_figures(out, a, b)
        assert R.g2_passes(out, a, b), figures
    e, t = figures[("six", True)]
    assert 1e-6 < t < 6e-6 and e < 1e-6, figures
    assert R.g2_passes(R.gemm(a, b, R.SIX), a, b)
    for products in (R.FIVE, R.THREE, ("hh",)):
        assert not R.g2_passes(R.gemm(a, b, products), a, b), products                      # even with exact accumulation
        assert not R.g2_passes(R.gemm(a, b, products, accumulate="fp32"), a, b), products
    # all nine products in float64 are the float64 GEMM itself: the pieces lose nothing
    s = a.double() @ b.double()
    assert R.rms(R.gemm(a, b, R.NINE) - s) / R.rms(s) < 1e-12


# ---------------------------------------------------------------- one reader of the switches: the route table and the keys
# (set_linear_impl, set_bf16) -> the constant of models/transformers.py that linear_route answers
ROUTE_TABLE = {("library", False): "LIBRARY_FP32", ("library", True): "LIBRARY_BF16", ("ftx", False): "LIBRARY_FP32", ("ftx", True): "OWN_BF16",
               ("ftx_split", False): "OWN_SPLIT", ("ftx_split", True): "OWN_SPLIT"}


def _image_branch():
    from fusiontransformer_amd.models.build import build_model
    from tests.helpers import small_cfg
    torch.manual_seed(0)
    net = build_model(small_cfg("middle"))[0].image_backbone
    assert len(net.backbone.blocks) == 2
    return net


def test_route_table_and_every_consumer_of_it(monkeypatch):
    """All six setter states on a depth-2 trunk: linear_route of the eight Linears is the documented table, and _linear, Mlp._fused_ftx,
    Mlp.forward's mode and native_image.modes each do what the route names."""
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd import native_image as ni
    from fusiontransformer_amd.models import transformers as T
    net = _image_branch()
    b = net.backbone
    xc = torch.zeros(1, 5, 768).as_subclass(_Cuda)
    routed = []

    def stub(name, what):
        def call(*a, **k):
            routed.append((name, what(a, k)))
            return a[0].new_zeros(*a[0].shape[:-1], (a[3] if name == "vit_mlp" else a[1]).shape[0])
        return call
    monkeypatch.setattr(spf, "vit_linear", stub("vit_linear", lambda a, k: k["mode"]))
    monkeypatch.setattr(spf, "vit_mlp", stub("vit_mlp", lambda a, k: k["mode"]))
    monkeypatch.setattr(T._LinearFn, "apply", staticmethod(stub("library", lambda a, k: a[3])))
    callee = {T.LIBRARY_FP32: ("library", False), T.LIBRARY_BF16: ("library", True), T.OWN_BF16: ("vit_linear", "bf16"), T.OWN_SPLIT: ("vit_linear", "split")}
    native = {T.OWN_BF16: ni.LINEAR_BF16, T.OWN_SPLIT: ni.LINEAR_SPLIT}
    assert len(set(callee)) == 4
    for (impl, on), name in ROUTE_TABLE.items():
        b.set_linear_impl(impl)
        b.set_bf16(on)
        want = getattr(T, name)
        assert [T.linear_route(lin) for lin in _lins(b)] == [want] * 8, (impl, on)
        for blk in b.blocks:
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1):
                del routed[:]
                T._linear(xc, lin)
                assert routed == [callee[want]], (impl, on, routed)
            del routed[:]
            T._linear(torch.zeros(1, 5, 3072).as_subclass(_Cuda), blk.mlp.fc2, with_bias=False)
            assert routed == [callee[want]], (impl, on, routed)
            own = want in native
            assert bool(blk.mlp._fused_ftx(xc)) is own, (impl, on)
            del routed[:]
            blk.mlp(xc)
            assert routed == ([("vit_mlp", callee[want][1])] if own else [callee[want]] * 2), (impl, on, routed)
        if own:
            assert ni.modes(net) == (native[want], ni.ATTN_FP32), (impl, on)
        else:
            with pytest.raises(ni.Unsupported, match="set_bf16" if impl == "ftx" else "library"):
                ni.modes(net)


def test_every_linears_switches_reach_both_graph_keys_and_the_table_signature(monkeypatch):
    """Flipping ftx_bf16 or ftx_linear_impl of ONE Linear of a block changes _graph_key, _infer_key and NativeImage._signature, and
    restoring it restores them.  Before the keys were built from block_switches this failed for ftx_bf16 of attn.proj and of mlp.fc2 on
    both graph keys: they recorded ftx_bf16 of attn.qkv and mlp.fc1 only, so a captured graph would have replayed the old kernels."""
    from fusiontransformer_amd import native_image as ni
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)   # the keys record the device; no GPU is touched here
    net = _image_branch()
    b = net.backbone
    b.set_bf16(False)
    ex = ni.NativeImage(net)
    x = torch.zeros(1, 3, 384, 384)

    def keys():
        return b._graph_key(x), b._infer_key(x), ex._signature()
    base = keys()
    blk = b.blocks[0]
    for name, lin in (("qkv", blk.attn.qkv), ("proj", blk.attn.proj), ("fc1", blk.mlp.fc1), ("fc2", blk.mlp.fc2)):
        for attr, other in (("ftx_bf16", True), ("ftx_linear_impl", "ftx_split")):
            was = getattr(lin, attr)
            assert was != other
            setattr(lin, attr, other)
            assert [new != old for new, old in zip(keys(), base)] == [True] * 3, (name, attr)
            setattr(lin, attr, was)
            assert keys() == base, (name, attr)
