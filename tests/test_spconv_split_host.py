"""Three-piece split sparse convolution (csrc/ftx_spconv_split.hip, cfg.MODEL.lidar_split) without a GPU: the two gates of its GPU
tests applied to emulations (they can fail: the six-product scheme passes, five or three products and bf16-rounded operands do
not); the C entry points exist, state their precision contract and refuse bad arguments before anything is launched; the column rule
is the fp32 family's; the weight-gradient occupancy table matches the code object; the model switch flags exactly the LiDAR branch's
GEMMs; the program checker takes operand mode 2, the output-stationary route included, and refuses mode 3 by name."""
import ctypes
import os
import re

import pytest
import torch

from fusiontransformer_amd import _lib
from fusiontransformer_amd import native_eval as ne
from tests import spconv_regimes as S
from tests import spconv_split_ref as SR
from tests import split_ref as R
from tests.norm_ref import gen, randn
from tests.test_cabi import ROOT, declared_symbols
from tests.test_native_program_host import CONV3, EVAL, TRAIN, accepted, answers, both, programs, refused, set_route, setter  # noqa: F401
from tests.test_spconv_regimes_gpu import GEMM_CASES, random_sizes

FAKE = ctypes.c_void_p(4096)   # never dereferenced: every call below must fail its argument check first
ENTRIES = ("ftx_spconv_pairs_gemm_split", "ftx_spconv_pairs_gemm_scatter_split", "ftx_rows_gemm_split", "ftx_spconv_pairs_wgrad_split",
           "ftx_spconv_pairs_wgrad_split_workspace_bytes", "ftx_spconv_gemm_split_block_cols", "ftx_spconv_wgrad_split_table_blocks")


# ---------------------------------------------------------------- the gates on emulations
@pytest.fixture(scope="module", params=[(36, 20), (100, 64)], ids=["36->20", "100->64"])
def layer(request, ftx_lib):
    """A synthetic 27-offset pair list of 6 000 pairs with its float64 references, shared by the gate tests of one layer."""
    ca, co = request.param
    g = gen(ca * 7 + co)
    sizes = random_sizes(g, 6000, 27)
    n_src, n_dst = 1500, max(sizes) + 17
    src, dst, koff = SR.host_pair_list(g, sizes, n_src, n_dst)
    A, W, G = randn(g, n_src, ca), randn(g, 27, ca, co, scale=(ca * 27) ** -0.5), randn(g, n_dst, co)
    length = SR.split_tile_len(ftx_lib, 6000, ca, co, 27)
    conv = SR.conv_gate(A, W, src, dst, koff, n_dst) + (SR.conv_products(A, W, src, dst, koff, n_dst, R.FIVE),)
    wgrad = SR.wgrad_gate(A, src, G, dst, koff, length) + (SR.wgrad_products(A, src, G, dst, koff, R.FIVE),)
    assert conv[0].numel() >= SR.G2_MIN_ELEMENTS and wgrad[0].numel() >= SR.G2_MIN_ELEMENTS
    return dict(A=A, W=W, G=G, src=src, dst=dst, koff=koff, n_dst=n_dst, length=length, conv=conv, wgrad=wgrad)


def _emulated(layer, **kw):
    e = layer
    return (SR.conv_emulated(e["A"], e["W"], e["src"], e["dst"], e["koff"], e["n_dst"], **kw),
            SR.wgrad_emulated(e["A"], e["src"], e["G"], e["dst"], e["koff"], e["length"], **kw))


def test_six_product_emulation_passes_both_gates(layer):
    for name, got, (ref, bound, s5) in zip(("conv", "wgrad"), _emulated(layer), (layer["conv"], layer["wgrad"])):
        r, (e, t) = SR.g1_ratio(got, ref, bound), SR.g2_figures(got, ref, s5)
        print(f"\n{name}: six products, G1 error / bound {r:.3g}, G2 E / T {e / t:.3g}")
        assert r <= 1.0, (name, r)
        assert e <= t / 2, (name, e, t)


@pytest.mark.parametrize("products", [R.FIVE, R.THREE], ids=["five", "three"])
def test_fewer_products_fail_g2(layer, products):
    for name, got, (ref, bound, s5) in zip(("conv", "wgrad"), _emulated(layer, products=products), (layer["conv"], layer["wgrad"])):
        assert not SR.g2_passes(got, ref, s5), name


def test_bf16_rounded_operands_fail_both_gates(layer):
    for name, got, (ref, bound, s5) in zip(("conv", "wgrad"), _emulated(layer, rounded=True), (layer["conv"], layer["wgrad"])):
        assert SR.g1_ratio(got, ref, bound) > 1.0, name
        assert not SR.g2_passes(got, ref, s5), name


# ---------------------------------------------------------------- host checks
def test_split_entries_are_exported_and_declared(ftx_lib):
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(ftx_lib, name), name
    # each entry takes exactly the arguments of its fp32 twin
    for name in ENTRIES[:5]:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_split", "")], name


def test_header_states_the_precision_contract():
    text = open(f"{ROOT}/include/ftx.h").read()
    m = re.search(r"/\* fp32-accurate sparse convolution on the bf16 MFMA.*?\*/", text, re.S)
    assert m, "the split sparse-conv paragraph is in include/ftx.h"
    para = " ".join(m.group(0).replace("\n *", " ").split())
    assert "h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m)" in para and "round-to-nearest-even" in para
    assert "both subtractions in fp32" in para and "If h is not finite, m = l = 0" in para
    assert "hh, hm, mh, hl, lh, mm" in para and "2.01 * 2^-24 * |a b|" in para
    assert "two fp32 accumulators per output element" in para and "mm, hl, lh, hm, mh in that order (smallest first)" in para
    assert "added once" in para and "No atomics" in para and "deterministic" in para and "not bit-identical" in para
    assert "`tmp`" in para and "ftx_spconv_reduce_bn_eval consume it unchanged" in para and "wgrad_reduce_kernel in tile order" in para
    # one definition of the split for both families
    csrc = os.path.join(ROOT, "fusiontransformer_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip"))]
    defs = [f for f in sources if re.search(r"void split1\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["ftx_split.h"], defs
    for f in ("ftx_dense_split.hip", "ftx_spconv_split.hip"):
        assert '#include "ftx_split.h"' in open(os.path.join(csrc, f)).read(), f


def test_pair_gemm_entries_refuse_bad_arguments(ftx_lib):
    L = ftx_lib
    assert L.ftx_spconv_pairs_gemm_split(FAKE, 100, FAKE, FAKE, 0, FAKE, 50, 6, 32, 27, FAKE, None) == -1
    assert b"ftx_spconv_pairs_gemm_split: channels must be multiples of 4" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_gemm_split(FAKE, 100, None, FAKE, 0, FAKE, 50, 32, 32, 27, FAKE, None) == -1
    assert b"ftx_spconv_pairs_gemm_split: null pointer" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_gemm_split(FAKE, 100, FAKE, FAKE, 0, FAKE, 50, 32, 32, 65, FAKE, None) == -1
    assert b"bad size" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_gemm_scatter_split(FAKE, 100, FAKE, FAKE, FAKE, 0, FAKE, 50, 32, 30, 8, FAKE, 50, None) == -1
    assert b"ftx_spconv_pairs_gemm_scatter_split: channels must be multiples of 4" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_gemm_scatter_split(FAKE, 100, FAKE, None, FAKE, 0, FAKE, 50, 32, 32, 8, FAKE, 50, None) == -1
    assert b"ftx_spconv_pairs_gemm_scatter_split: null pointer" in L.ftx_last_error()
    assert L.ftx_rows_gemm_split(FAKE, 100, FAKE, 0, None, 32, 22, FAKE, None) == -1
    assert b"ftx_rows_gemm_split: channels must be multiples of 4" in L.ftx_last_error()
    assert L.ftx_rows_gemm_split(FAKE, 100, None, 0, None, 32, 32, FAKE, None) == -1
    assert b"ftx_rows_gemm_split: null pointer" in L.ftx_last_error()
    # empty inputs are no-ops, as for the fp32 entries
    assert L.ftx_spconv_pairs_gemm_split(None, 0, None, None, 0, None, 0, 32, 32, 27, None, None) == 0
    assert L.ftx_rows_gemm_split(None, 0, None, 0, None, 32, 32, None, None) == 0


def test_wgrad_entry_refuses_bad_arguments_and_short_workspace(ftx_lib):
    L = ftx_lib
    P, ca, cg, kvol = 382735, 128, 96, 27
    ws = L.ftx_spconv_pairs_wgrad_split_workspace_bytes(P, ca, cg, kvol)
    assert ws > 0 and ws == L.ftx_spconv_pairs_wgrad_split_workspace_bytes(P, ca, cg, kvol)
    assert ws % (4 * ca * cg) == 0 and ws // (4 * ca * cg) > kvol
    args = lambda a, ca_=ca, dw=FAKE, w=ws: (a, 81237, FAKE, FAKE, 81237, FAKE, FAKE, P, ca_, cg, kvol, dw, FAKE, w, None)   # noqa: E731
    assert L.ftx_spconv_pairs_wgrad_split(*args(FAKE, ca_=126)) == -1
    assert b"ftx_spconv_pairs_wgrad_split: channels must be multiples of 4" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_wgrad_split(*args(None)) == -1
    assert b"ftx_spconv_pairs_wgrad_split: null pointer" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_wgrad_split(*args(FAKE, dw=None)) == -1
    assert b"ftx_spconv_pairs_wgrad_split: null dW" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_wgrad_split(*args(FAKE, w=ws - 1)) == -3
    assert b"ftx_spconv_pairs_wgrad_split: workspace" in L.ftx_last_error()
    # dense mode needs all three index pointers null
    assert L.ftx_spconv_pairs_wgrad_split(FAKE, 100, None, FAKE, 100, FAKE, None, 100, 32, 32, 1, FAKE, FAKE, 1 << 20, None) == -1
    assert b"must be all set or all null" in L.ftx_last_error()
    # the tile length this family's table and step give is the one its workspace query is sized for
    for n, a, g, k in ((P, ca, cg, kvol), (6000, 36, 20, 27), (81237, 256, 32, 1), (30000, 100, 132, 27)):
        assert SR.split_tile_len(L, n, a, g, k) % 64 == 0


def test_block_cols_equal_the_fp32_query(ftx_lib):
    L = ftx_lib
    assert L.ftx_spconv_gemm_split_block_cols(6, 100, 27) == -1
    for e in S.PRODUCTION:
        kvol = 27 if e["map"][0] == "subm" else 8
        for c, want in ((e["co"], e["fwd"]), (e["ca"], e["dgrad"])):
            assert L.ftx_spconv_gemm_split_block_cols(c, e["n_pairs"], kvol) == L.ftx_spconv_gemm_block_cols(c, e["n_pairs"], kvol) == want, e["name"]
    for e in S.DENSE:
        for c, want in ((e["co"], e["fwd"]), (e["ca"], e["dgrad"])):
            assert L.ftx_spconv_gemm_split_block_cols(c, e["rows"], 0) == L.ftx_spconv_gemm_block_cols(c, e["rows"], 0) == want, e["name"]
    for ca, co, n_pairs, cols in GEMM_CASES:
        assert L.ftx_spconv_gemm_split_block_cols(co, n_pairs, 27) == L.ftx_spconv_gemm_block_cols(co, n_pairs, 27) == cols


def test_split_wgrad_occupancy_table_matches_the_code_object():
    """The table in csrc/ftx_spconv_split.hip against the registers / LDS the compiler allocated: min(8, 512 / VGPRs rounded up to 8,
    160 KiB / LDS), as tests/test_spconv_bf16_host.py checks the bf16 table.  No instantiation of either split kernel uses scratch,
    and none passes the 64 KB of static LDS.  A stale table costs speed only, never results."""
    import subprocess
    import tempfile
    bundler, readelf = "/opt/rocm/lib/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    src = os.path.join(ROOT, "fusiontransformer_amd", "csrc", "ftx_spconv_split.hip")
    if not (os.path.exists(bundler) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools are not here")
    lib = _lib.load()
    with tempfile.TemporaryDirectory() as d:
        dev = os.path.join(d, "dev.o")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", dev],
                       check=True, cwd=d)
        co = os.path.join(d, "k.co")
        subprocess.run([bundler, "--unbundle", "--type=o", "--input=" + dev, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
    seen = gemms = 0
    for blk in notes.split("- .agpr_count")[1:]:
        if "_split_kernel" not in blk:
            continue
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, "scratch"
        assert lds <= 64 * 1024
        m = re.search(r"pairs_wgrad_split_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)E", blk)
        if not m:
            gemms += "pairs_gemm_split_kernel" in blk
            continue
        mi, ni, wmg, wng = (int(x) for x in m.groups())
        vg = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        occ = min(8, 512 // ((vg + 7) // 8 * 8), (160 * 1024) // lds)
        assert lib.ftx_spconv_wgrad_split_table_blocks(mi, wmg, ni, wng) == occ, ((mi, ni, wmg, wng), vg, lds, occ)
        seen += 1
    assert seen == 16 and gemms == 4
    assert lib.ftx_spconv_wgrad_split_table_blocks(4, 1, 1, 1) == -1


# ---------------------------------------------------------------- the model switch
def _lidar(kind="middle", **switches):
    from fusiontransformer_amd.models.build import build_model
    from tests.helpers import small_cfg
    cfg = small_cfg(kind)
    for k, v in switches.items():
        cfg.MODEL[k] = v
    torch.manual_seed(0)
    model, _, _ = build_model(cfg)
    return model.lidar_backbone


def _flagged(lb):
    from fusiontransformer_amd.models.spvcnn import Conv3d
    convs = [m for m in lb.modules() if isinstance(m, Conv3d)]
    linears = {n: m for n, m in lb.named_modules() if isinstance(m, torch.nn.Linear)}
    return convs, linears


@pytest.mark.parametrize("kind,transform", [("middle", "middle_fusion_transform"), ("early", "early_fusion_transform")])
def test_lidar_split_flags_the_lidar_gemms_and_no_head(kind, transform):
    from fusiontransformer_amd.models.spvcnn import bf16_operands, operand_mode
    lb = _lidar(kind, lidar_split=True)
    convs, linears = _flagged(lb)
    assert len(convs) > 40 and all(operand_mode(c) == "split" and not bf16_operands(c) for c in convs)
    want = {"point_transforms.0.0", "point_transforms.1.0", "point_transforms.2.0", transform + ".0"}
    assert {n for n, m in linears.items() if operand_mode(m) == "split"} == want
    assert operand_mode(lb.linear) == "fp32" and operand_mode(lb.linear2) == "fp32"
    assert lb.lidar_split and not lb.lidar_bf16
    # exactly the modules set_bf16 flags
    split = {id(m) for m in lb.modules() if operand_mode(m) == "split"}
    lb.set_split(False)
    assert not lb.lidar_split and all(operand_mode(m) == "fp32" for m in lb.modules())
    lb.set_bf16(True)
    assert {id(m) for m in lb.modules() if bf16_operands(m)} == split


def test_default_build_flags_nothing():
    from fusiontransformer_amd.config import get_cfg_defaults
    from fusiontransformer_amd.models.spvcnn import operand_mode
    lb = _lidar()
    assert not lb.lidar_split and not lb.lidar_bf16
    assert all(operand_mode(m) == "fp32" for m in lb.modules())
    assert get_cfg_defaults().MODEL.lidar_split is False and get_cfg_defaults().MODEL.lidar_bf16 is False


def test_both_switches_together_raise():
    with pytest.raises(ValueError, match="lidar_bf16 and lidar_split"):
        _lidar(lidar_bf16=True, lidar_split=True)
    lb = _lidar(lidar_split=True)
    with pytest.raises(ValueError, match="lidar_bf16 and lidar_split"):
        lb.set_bf16(True)
    lb = _lidar(lidar_bf16=True)
    with pytest.raises(ValueError, match="lidar_bf16 and lidar_split"):
        lb.set_split(True)
    assert lb.lidar_bf16 and not lb.lidar_split


def test_functional_operand_modes():
    from fusiontransformer_amd import functional as spf
    assert (spf.operand_mode(), spf.operand_mode(True), spf.operand_mode(False, "split"), spf.operand_mode(True, "bf16")) == (0, 1, 2, 1)
    assert spf.operand_mode(operands="fp32") == 0 and spf.OPERANDS == {"fp32": 0, "bf16": 1, "split": 2}
    for bad in (dict(operands="fp16"), dict(bf16=True, operands="split"), dict(bf16=3), dict(bf16=2)):      # bf16 is a flag: 2 never means split
        with pytest.raises(ValueError):
            spf.operand_mode(**bad)
    # the tables answer bf16=False / True as they always did, and the third family next to them
    assert spf._PAIRS_GEMM[False] == ("ftx_spconv_pairs_gemm", "spconv_pairs_gemm") and spf._PAIRS_GEMM[True][1] == "spconv_pairs_gemm_bf16"
    assert spf._PAIRS_GEMM[spf.SPLIT] == ("ftx_spconv_pairs_gemm_split", "spconv_pairs_gemm_split")
    assert spf._PAIRS_WGRAD[spf.SPLIT][::2] == ("ftx_spconv_pairs_wgrad_split", "spconv_pairs_wgrad_split")
    assert spf._PAIRS_GEMM_SCATTER[spf.SPLIT] == "ftx_spconv_pairs_gemm_scatter_split" and spf._ROWS_GEMM[spf.SPLIT] == "ftx_rows_gemm_split"


def test_layer_table_and_cache_key_carry_the_mode():
    from fusiontransformer_amd.models.spvcnn import SPVCNN
    torch.manual_seed(0)
    net = SPVCNN(lidar_split=True)
    host = ne._Host(ne.emit_program(net))
    assert all(int(r["bf16"]) == 2 for r in host.model_table())
    key = host.key
    net.set_split(False)
    assert all(int(r["bf16"]) == 0 for r in host.model_table()) and host.key != key
    net.set_bf16(True)
    assert all(int(r["bf16"]) == 1 for r in host.model_table())


# ---------------------------------------------------------------- the program checker
def _all_layers(mode):
    def mutate(t):
        t["layers"]["bf16"] = mode
    return mutate


def test_checker_accepts_mode_2_ostat_route_included(ftx_lib, programs):
    for a in answers(ftx_lib, *both(programs, _all_layers(2))):
        assert accepted(a), a
    ostat = set_route(CONV3, ne.ROUTES["ostat"])
    for mode in (0, 2):
        for a in answers(ftx_lib, *both(programs, lambda t, m=mode: (_all_layers(m)(t), ostat(t)))):
            assert accepted(a), (mode, a)
    # a bf16 layer never takes the exact-fp32 kernel
    text = "op 6 (conv_bn) layer 3: the output-stationary route does not take this layer"
    ev, fwd, bwd = answers(ftx_lib, *both(programs, lambda t: (_all_layers(1)(t), ostat(t))))
    assert refused(ev, EVAL + text) and refused(fwd, TRAIN + text) and refused(bwd, TRAIN + text)


@pytest.mark.parametrize("mode", [3, -1])
def test_checker_refuses_an_unknown_mode_with_the_layer_named(ftx_lib, programs, mode):
    text = f"op 6 (conv_bn) layer 3: operand mode {mode} is not 0 (fp32), 1 (bf16) or 2 (split)"
    ev, fwd, bwd = answers(ftx_lib, *both(programs, setter("layers", 3, "bf16", mode)))
    assert refused(ev, EVAL + text), ev
    assert refused(fwd, TRAIN + text) and refused(bwd, TRAIN + text), (fwd, bwd)
