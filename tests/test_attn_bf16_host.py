"""bf16-operand attention without a GPU: the C entry points exist and refuse bad arguments before anything is launched, and the
model layer carries attn_impl="ftx_bf16" to every block and into the trunk's graph keys.

And the bf16 bars of tests/attn_ref.py without a GPU: a numpy model of the bf16-operand attention kernels' arithmetic
(attn_ref.emulate_bf16: the precision contract of csrc/ftx_attn.hip step by step) stays inside them, and each defect they exist for,
planted into that model, is thrown out: the structural ones of the fp32 kernels and three breaches of the contract that only lse
shows.  The GPU tests (tests/test_attn_bf16_gpu.py) hold the real kernels to the same bars.

The motive: the two constants the bf16 kernels were held to before (OUT_TOL, a max-abs on out, and GRAD_TOL, a relative L2 over a
whole gradient) accept one zero key of the ragged tile let through the mask at the ViT's 578 tokens; the bars do not
(test_the_constants_accept_an_unmasked_key_the_bars_do_not)."""
import ctypes
import functools
import re

import pytest
import torch

from fusiontransformer_amd import _lib
from tests import attn_ref as R
from tests.test_attn_bf16_gpu import GRAD_TOL, OUT_TOL      # the constants only: nothing of that module runs here
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


# ---------------------------------------------------------------- the bars of tests/attn_ref.py
SCALE = 0.125
CONTRACT = ("operands_truncated", "scale_folded_into_q", "rowsum_of_rounded_p")


@functools.lru_cache(maxsize=None)
def case(kind, T, scale=SCALE):
    return R.CaseBf16(kind, 2, T, 2, scale)


def inside(c, label, **kw):
    r, E = c.ratios(R.emulate_bf16(c.qkv, c.go, c.scale, **kw))
    print(R.format_row(f"emulated {label} max|lse|={c.max_lse:.0f}", c.E_bar, E, r))
    return r


@pytest.mark.parametrize("T", [1, 2, 31, 33, 70, 129, 257, 578])
@pytest.mark.parametrize("kind", ["gauss", "peaked", "large"])
def test_emulated_kernels_stay_inside_the_bars(kind, T):
    c = case(kind, T)
    for split in (1, 8):
        r = inside(c, f"{kind} T={T} split={split}", split=split)
        assert R.worst(r) <= 1.0, (kind, T, split, r)


@pytest.mark.parametrize("T", [70, 257, 290])
@pytest.mark.parametrize("kind", ["ascending", "late_max"])
def test_emulated_kernels_stay_inside_the_bars_on_the_constructed_inputs(kind, T):
    c = case(kind, T)
    for split in (1, 8):
        r = inside(c, f"{kind} T={T} split={split}", split=split)
        assert R.worst(r) <= 1.0, (kind, T, split, r)


def rejected(fault, kind, T, scale=SCALE):
    c = case(kind, T, scale)
    r, E = c.ratios(R.emulate_bf16(c.qkv, c.go, scale, 1, fault=fault))
    print(f"{fault} {kind} T={T} scale={scale}: " + " ".join(f"{n} {max(v):.3g}" for n, v in r.items()))
    return r


@pytest.mark.parametrize("T", [70, 257])
@pytest.mark.parametrize("kind", ["gauss", "peaked"])
@pytest.mark.parametrize("fault", R.FAULTS_BF16)
def test_bars_reject_planted_faults(fault, kind, T):
    """Each fault must exceed the bar on at least one tensor.  Without the fault (fault=None) every one of these cases fails: the
    unplanted model is inside the bars (the tests above)."""
    r = rejected(fault, kind, T)
    assert R.worst(r) > 1.0, (fault, kind, T, r)


@pytest.mark.parametrize("kind", ["gauss", "peaked"])
def test_bars_reject_an_unmasked_key_at_the_vit_token_count(kind):
    r = rejected("extra_zero_key", kind, 578)
    assert R.worst(r) > 1.0, (kind, r)


@pytest.mark.parametrize("T", [70, 257])
@pytest.mark.parametrize("kind", ["gauss", "peaked"])
@pytest.mark.parametrize("fault", CONTRACT)
def test_lse_bar_rejects_contract_faults_at_a_scale_that_is_no_power_of_two(fault, kind, T):
    """scale 0.1.  The kernels work with sl2 = scale * log2e, which is exact in bf16 at no scale, but a kernel that folded the scale
    alone into Q would be exact at 0.125 and at every other power of two: only a scale like 0.1 tells the two apart on the card, so
    the bars have to work there too.  The unplanted model is inside the bars at this scale; each breach shows in lse."""
    c = case(kind, T, 0.1)
    assert R.worst(inside(c, f"{kind} T={T} scale=0.1", split=1)) <= 1.0
    r = rejected(fault, kind, T, 0.1)
    assert max(r["lse"]) > 1.0, (fault, kind, T, r)


def test_contract_faults_show_in_lse():
    for fault in CONTRACT:
        for kind in ("gauss", "peaked"):
            assert max(rejected(fault, kind, 257)["lse"]) > 1.0, (fault, kind)


def test_the_constants_accept_an_unmasked_key_the_bars_do_not():
    """One zero key of the ragged tile let through the mask, at the ViT's T = 578 on the flat "gauss" inputs (the inputs the constants
    were applied to): max-abs of out and the relative L2 of every gradient are inside OUT_TOL / GRAD_TOL, and the same result is over
    the bars."""
    c = case("gauss", 578)
    got = R.emulate_bf16(c.qkv, c.go, SCALE, 2, fault="extra_zero_key")
    out, _, g = (torch.from_numpy(x).double() for x in got)
    ref_out, _, ref_g = c.ref64
    err_out = float((out - ref_out).abs().max())
    errs = [float((g[:, :, i] - ref_g[:, :, i]).norm() / ref_g[:, :, i].norm()) for i in range(3)]
    r, _ = c.ratios(got)
    print(f"extra_zero_key gauss T=578: out {err_out:.2e} (OUT_TOL {OUT_TOL}), gradient L2 {max(errs):.2e} (GRAD_TOL {GRAD_TOL}), "
          f"worst ratio to the bars {R.worst(r):.3g}")
    assert err_out <= OUT_TOL and max(errs) <= GRAD_TOL
    assert R.worst(r) > 1.0, r


def test_bar_is_built_from_the_yardstick_and_the_rounding_counts():
    E_yard = {n: (1e-4, 3e-4) for n in R.TENSORS}
    E32_lse = (1e-8, 3e-8)
    b = R.bar_bf16(E_yard, E32_lse, 40.0)
    assert b["dv"] == (4 * 1e-4 + 4 * R.U * 40.0, 4 * 3e-4 + 4 * R.U * 40.0) and b["out"] == b["dq"] == b["dk"] == b["dv"]
    assert b["lse"] == (4 * 1e-8 + 8 * R.U, 4 * 3e-8 + 8 * R.U)                     # the fp32 bar: E_yard["lse"] plays no part
    assert R.bar_bf16(E_yard, E32_lse, 0.25)["out"] == (4 * 1e-4 + 4 * R.U, 4 * 3e-4 + 4 * R.U)      # max(1, |lse|)
    assert b["lse"] == R.bar({n: E32_lse for n in R.TENSORS}, 40.0)["lse"]
    zero = R.bar_bf16({n: (0.0, 0.0) for n in R.TENSORS}, (0.0, 0.0), 0.0)
    assert all(v > 0 for pair in zero.values() for v in pair)                       # T = 1: the yardstick is exact


def test_yardstick_states_the_contract():
    """The yardstick's lse is the reference's (nothing on the way to it is rounded); its out and gradients differ from the reference by
    the two operand roundings, 2^-9 relative each, and by no more; rounded() is bf16 round-to-nearest-even."""
    c = case("gauss", 70)
    assert c.E_yard["lse"] == (0.0, 0.0)
    for n in ("out", "dq", "dk", "dv"):
        assert 0 < c.E_yard[n][1] <= 2 * 2.0 ** -9, (n, c.E_yard[n])
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8)], dtype=torch.float32)
    assert R.rounded(x).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0]         # ties go to the even mantissa
    assert R.rounded(x.numpy()).dtype == torch.float64
