"""bf16-operand sparse convolution without a GPU: the C entry points exist, state their precision contract and refuse bad arguments
before anything is launched; the bf16 weight-gradient occupancy table matches the code object; the model switch flags exactly the
LiDAR branch's GEMMs."""
import ctypes
import os
import re

import pytest
import torch

from fusiontransformer_amd import _lib
from tests.test_cabi import ROOT, declared_symbols

FAKE = ctypes.c_void_p(4096)   # never dereferenced: every call below must fail its argument check first
ENTRIES = ("ftx_spconv_pairs_gemm_bf16", "ftx_spconv_pairs_gemm_scatter_bf16", "ftx_rows_gemm_bf16", "ftx_spconv_pairs_wgrad_bf16",
           "ftx_spconv_pairs_wgrad_bf16_workspace_bytes", "ftx_spconv_gemm_bf16_block_cols", "ftx_spconv_wgrad_bf16_table_blocks")


def test_bf16_entries_are_exported_and_declared(ftx_lib):
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(ftx_lib, name), name
    # each entry takes exactly the arguments of its fp32 twin
    for name in ENTRIES[:5]:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_bf16", "")], name


def test_header_states_the_precision_contract():
    text = open(f"{ROOT}/include/ftx.h").read()
    m = re.search(r"/\* bf16-operand sparse convolution.*?\*/", text, re.S)
    assert m, "the bf16 sparse-conv paragraph is in include/ftx.h"
    para = " ".join(m.group(0).split())
    assert "round-to-nearest-even" in para and "from their stored fp32 values" in para
    assert "Accumulation is fp32" in para and "all storage stays fp32" in para
    assert "`tmp`" in para and "deterministic" in para


def test_pair_gemm_entries_refuse_bad_arguments(ftx_lib):
    L = ftx_lib
    assert L.ftx_spconv_pairs_gemm_bf16(FAKE, 100, FAKE, FAKE, 0, FAKE, 50, 6, 32, 27, FAKE, None) == -1
    assert b"ftx_spconv_pairs_gemm_bf16: channels must be multiples of 4" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_gemm_bf16(FAKE, 100, None, FAKE, 0, FAKE, 50, 32, 32, 27, FAKE, None) == -1
    assert b"ftx_spconv_pairs_gemm_bf16: null pointer" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_gemm_bf16(FAKE, 100, FAKE, FAKE, 0, FAKE, 50, 32, 32, 65, FAKE, None) == -1
    assert b"bad size" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_gemm_scatter_bf16(FAKE, 100, FAKE, FAKE, FAKE, 0, FAKE, 50, 32, 30, 8, FAKE, 50, None) == -1
    assert b"ftx_spconv_pairs_gemm_scatter_bf16: channels must be multiples of 4" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_gemm_scatter_bf16(FAKE, 100, FAKE, None, FAKE, 0, FAKE, 50, 32, 32, 8, FAKE, 50, None) == -1
    assert b"ftx_spconv_pairs_gemm_scatter_bf16: null pointer" in L.ftx_last_error()
    assert L.ftx_rows_gemm_bf16(FAKE, 100, FAKE, 0, None, 32, 22, FAKE, None) == -1
    assert b"ftx_rows_gemm_bf16: channels must be multiples of 4" in L.ftx_last_error()
    assert L.ftx_rows_gemm_bf16(FAKE, 100, None, 0, None, 32, 32, FAKE, None) == -1
    assert b"ftx_rows_gemm_bf16: null pointer" in L.ftx_last_error()
    # empty inputs are no-ops, as for the fp32 entries
    assert L.ftx_spconv_pairs_gemm_bf16(None, 0, None, None, 0, None, 0, 32, 32, 27, None, None) == 0
    assert L.ftx_rows_gemm_bf16(None, 0, None, 0, None, 32, 32, None, None) == 0


def test_wgrad_entry_refuses_bad_arguments_and_short_workspace(ftx_lib):
    L = ftx_lib
    P, ca, cg, kvol = 382735, 128, 96, 27
    ws = L.ftx_spconv_pairs_wgrad_bf16_workspace_bytes(P, ca, cg, kvol)
    assert ws > 0 and ws == L.ftx_spconv_pairs_wgrad_bf16_workspace_bytes(P, ca, cg, kvol)
    assert ws % (4 * ca * cg) == 0 and ws // (4 * ca * cg) > kvol
    args = lambda a, ca_=ca, dw=FAKE, w=ws: (a, 81237, FAKE, FAKE, 81237, FAKE, FAKE, P, ca_, cg, kvol, dw, FAKE, w, None)   # noqa: E731
    assert L.ftx_spconv_pairs_wgrad_bf16(*args(FAKE, ca_=126)) == -1
    assert b"ftx_spconv_pairs_wgrad_bf16: channels must be multiples of 4" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_wgrad_bf16(*args(None)) == -1
    assert b"ftx_spconv_pairs_wgrad_bf16: null pointer" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_wgrad_bf16(*args(FAKE, dw=None)) == -1
    assert b"ftx_spconv_pairs_wgrad_bf16: null dW" in L.ftx_last_error()
    assert L.ftx_spconv_pairs_wgrad_bf16(*args(FAKE, w=ws - 1)) == -3
    assert b"ftx_spconv_pairs_wgrad_bf16: workspace" in L.ftx_last_error()
    # dense mode needs all three index pointers null
    assert L.ftx_spconv_pairs_wgrad_bf16(FAKE, 100, None, FAKE, 100, FAKE, None, 100, 32, 32, 1, FAKE, FAKE, 1 << 20, None) == -1
    assert b"must be all set or all null" in L.ftx_last_error()


def test_block_cols_query(ftx_lib):
    L = ftx_lib
    assert L.ftx_spconv_gemm_bf16_block_cols(6, 100, 27) == -1
    for co, n, kvol in ((32, 382735, 27), (96, 382735, 27), (128, 126675, 27), (256, 20329, 27), (20, 81237, 0), (256, 81237, 0)):
        assert L.ftx_spconv_gemm_bf16_block_cols(co, n, kvol) in (32, 64, 96, 128)


def test_bf16_wgrad_occupancy_table_matches_the_code_object():
    """The table in csrc/ftx_spconv_bf16.hip against the registers / LDS the compiler allocated: min(8, 512 / VGPRs rounded up to 8,
    160 KiB / LDS), as tests/test_cabi.py checks the fp32 table.  A stale table costs speed only, never results."""
    import subprocess
    import tempfile
    bundler, readelf = "/opt/rocm/lib/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    src = os.path.join(ROOT, "fusiontransformer_amd", "csrc", "ftx_spconv_bf16.hip")
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
    seen = 0
    for blk in notes.split("- .agpr_count")[1:]:
        m = re.search(r"pairs_wgrad_bf16_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)E", blk)
        if not m:
            continue
        mi, ni, wmg, wng = (int(x) for x in m.groups())
        vg = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, ("scratch", mi, ni, wmg, wng)
        occ = min(8, 512 // ((vg + 7) // 8 * 8), (160 * 1024) // lds)
        assert lib.ftx_spconv_wgrad_bf16_table_blocks(mi, wmg, ni, wng) == occ, ((mi, ni, wmg, wng), vg, lds, occ)
        seen += 1
    assert seen == 16


def _lidar(lidar_bf16=None, kind="middle"):
    from fusiontransformer_amd.models.build import build_model
    from tests.helpers import small_cfg
    cfg = small_cfg(kind)
    if lidar_bf16 is not None:
        cfg.MODEL.lidar_bf16 = lidar_bf16
    torch.manual_seed(0)
    model, _, _ = build_model(cfg)
    return model.lidar_backbone


def _flagged(lb):
    from fusiontransformer_amd.models.spvcnn import Conv3d
    convs = [m for m in lb.modules() if isinstance(m, Conv3d)]
    linears = {n: m for n, m in lb.named_modules() if isinstance(m, torch.nn.Linear)}
    return convs, linears


@pytest.mark.parametrize("kind,transform", [("middle", "middle_fusion_transform"), ("early", "early_fusion_transform")])
def test_lidar_bf16_flags_the_lidar_gemms_and_no_head(kind, transform):
    lb = _lidar(True, kind)
    convs, linears = _flagged(lb)
    assert len(convs) > 40 and all(c.ftx_bf16 for c in convs)
    want = {"point_transforms.0.0", "point_transforms.1.0", "point_transforms.2.0", transform + ".0"}
    assert {n for n, m in linears.items() if getattr(m, "ftx_bf16", False)} == want
    assert not getattr(lb.linear, "ftx_bf16", False) and not getattr(lb.linear2, "ftx_bf16", False)
    assert lb.lidar_bf16
    lb.set_bf16(False)
    assert not any(c.ftx_bf16 for c in convs) and not any(getattr(m, "ftx_bf16", False) for m in linears.values())


def test_default_build_flags_nothing_whatever_the_environment(monkeypatch):
    lb = _lidar()
    convs, linears = _flagged(lb)
    assert not lb.lidar_bf16
    assert not any(getattr(c, "ftx_bf16", False) for c in convs)
    assert not any(getattr(m, "ftx_bf16", False) for m in linears.values())
    # only cfg.MODEL.lidar_bf16 chooses: FTX_LIDAR_BF16 (a switch since removed) left in the environment changes nothing
    monkeypatch.setenv("FTX_LIDAR_BF16", "1")
    assert not _lidar().lidar_bf16
    assert not _lidar(False).lidar_bf16
