"""The fp32 attention kernels (ftx_attn_fwd_tiled / ftx_attn_bwd_tiled) against float64 at every tile edge, inside bars computed at
run time from the float32 yardstick (tests/attn_ref.py: bar(E32, max|lse|); no tolerance in this file is a number), and the
structural properties of both kernel families: a (batch, head) slice never sees its neighbours (bitwise), the automatic tiling is
the documented explicit one (bitwise), nothing is read or written outside the operands (guard bands), results repeat run to run.

The bf16-operand kernels have their bars in tests/test_attn_bf16_gpu.py: check_against_rounded with OUT_TOL and GRAD_TOL, and
assert_inside_bf16_bars (bars from attn_ref.yardstick_bf16, as here from the float32 yardstick), which holds them at every tile edge
there; here the guard-band runs and the T = 1 case assert both.  At T = 1 the true dQ and dK are exactly 0 and a relative L2 against
them is undefined (the kernels' dS = P (dP - delta) is a difference of two differently ordered sums, a few ulp, not 0), so for GRAD_TOL
dQ and dK are there taken relative to attn_ref.abs_gradients, as the bars take them throughout.

Measured on an MI355X: profiles/attn_fp32_accuracy.txt."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_ref as R
from tests.test_attn_bf16_gpu import (GRAD_TOL, OUT_TOL, assert_inside_bf16_bars, case_bf16, check_against_rounded,
                                      reference as reference64, rel_l2, rounded)

pytestmark = pytest.mark.gpu

EXPLICIT = [(4, 2), (2, 2), (2, 4), (1, 2), (1, 4), (1, 8)]
TILINGS = [(0, 0)] + EXPLICIT
ENTRIES = {"fp32": ("ftx_attn_fwd_tiled", "ftx_attn_bwd_tiled"), "bf16": ("ftx_attn_fwd_bf16", "ftx_attn_bwd_bf16")}
EDGES = R.EDGES               # below one 32-token tile, its edges, the 4-wave block's edges, the ViT's T
B, H = 2, 3
GUARD = 256                   # floats on each side of a banded operand (keeps the 16-byte alignment of the rows)
SENTINEL = 0x7FA5A5A5         # a NaN with a payload: an output element that was never written is not finite, a band that was is changed


def _banded(shape, data=None):
    """A tensor of `shape` as a view into the middle of a larger allocation: (whole, view).  With data: NaN bands around a copy of it
    (an operand).  Without: the sentinel everywhere (an output)."""
    n = int(np.prod(shape))
    if data is None:
        whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        whole = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
        whole[GUARD:GUARD + n] = torch.from_numpy(np.ascontiguousarray(data)).reshape(-1).cuda()
    return whole, whole[GUARD:GUARD + n].view(shape)


def _bands_intact(whole):
    w = whole.view(torch.int32)
    return bool((w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all())


def launch(prec, qkv, go, scale, fwd=(0, 0), bwd=None, banded=False):
    """The two C entries directly (the autograd function hides lse): float32 CPU tensors out, lse, grad_qkv.  `bwd` = the backward's
    tiling (default: the forward's).  banded: every operand sits between guard bands; returns also whether the outputs' bands
    survived."""
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd._lib import check, ptr, stream
    L = _lib.load()
    f_fwd, f_bwd = (getattr(L, n) for n in ENTRIES[prec])
    bwd = fwd if bwd is None else bwd
    Bq, T, _, Hq, D = qkv.shape
    if banded:
        (_, x), (_, g) = _banded(qkv.shape, qkv), _banded(go.shape, go)
        (w_out, out), (w_lse, lse), (w_gq, gq) = _banded((Bq, T, Hq * D)), _banded((Bq, Hq, T)), _banded(qkv.shape)
    else:
        x, g = torch.from_numpy(qkv).cuda(), torch.from_numpy(go).cuda()
        out, lse, gq = torch.empty((Bq, T, Hq * D), device="cuda"), torch.empty((Bq, Hq, T), device="cuda"), torch.empty_like(x)
    ws_bytes = int(L.ftx_attn_bwd_workspace_bytes(Bq, T, Hq))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    check(f_fwd(ptr(x), Bq, T, Hq, D, float(scale), ptr(out), ptr(lse), fwd[0], fwd[1], stream()), "fwd")
    check(f_bwd(ptr(x), ptr(out), ptr(g), ptr(lse), Bq, T, Hq, D, float(scale), ptr(gq), ptr(ws), ws_bytes, bwd[0], bwd[1], stream()), "bwd")
    torch.cuda.synchronize()
    res = (out.cpu(), lse.cpu(), gq.cpu())
    return (res, all(_bands_intact(w) for w in (w_out, w_lse, w_gq))) if banded else res


def bitwise_equal(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _case(kind, T, scale, b, h):
    return R.Case(kind, b, T, h, scale)


def case(kind, T, scale=0.125, b=B, h=H):
    """Inputs, float64 reference, yardstick and bars: computed once and shared by every tiling."""
    return _case(kind, T, scale, b, h)


def assert_inside_bars(c, got, label):
    assert all(bool(torch.isfinite(x).all()) for x in got), label
    r, E = c.ratios(got)
    print(R.format_row(f"{label} max|lse|={c.max_lse:.0f}", c.E32, E, r))
    assert R.worst(r) <= 1.0, (label, r, E)


def bf16_inside_bars(got, qkv, go, scale, label):
    """check_against_rounded's assertions on results already in hand (T = 1: see the module docstring)."""
    out, lse, gq = (x.double() for x in got)
    assert all(bool(torch.isfinite(x).all()) for x in got), label
    ref_out, _, ref_g = reference64(rounded(qkv), rounded(go), scale)
    assert float((out - ref_out).abs().max()) <= OUT_TOL, label
    if qkv.shape[1] == 1:
        absg = R.abs_gradients(rounded(qkv), rounded(go), scale)
        errs = [float((gq[:, :, i] - ref_g[:, :, i]).norm() / absg[i].norm()) for i in range(2)] + [rel_l2(gq[:, :, 2], ref_g[:, :, 2])]
    else:
        errs = [rel_l2(gq[:, :, i], ref_g[:, :, i]) for i in range(3)]
    assert max(errs) <= GRAD_TOL, (label, errs)


# ---------------------------------------------------------------- accuracy (fp32)
ACCURACY = R.ACCURACY        # shared with tests/test_attn_bf16_gpu.py


@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("kind,T,scale", ACCURACY)
def test_fp32_matches_float64_inside_the_bars(kind, T, scale, tiling):
    c = case(kind, T, scale)
    assert_inside_bars(c, launch("fp32", c.qkv, c.go, scale, tiling), f"acc {kind} T={T} scale={scale} tiling={tiling}")


@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("T", [100, 578])
def test_fp32_large_logits_match_float64(T, tiling):
    """Scores around +-7000, |lse| up to ~5000: out, lse and every gradient against float64, inside the same bars."""
    c = case("large", T)
    assert_inside_bars(c, launch("fp32", c.qkv, c.go, 0.125, tiling), f"acc large T={T} scale=0.125 tiling={tiling}")


def test_fp32_autograd_path_is_the_same_launch():
    """functional.attention (what the model calls) gives bit for bit what the C entries give, so the bars hold for it."""
    from fusiontransformer_amd import functional as spf
    c = case("peaked", 129)
    x = torch.from_numpy(c.qkv).cuda().requires_grad_(True)
    out = spf.attention(x, 0.125)
    out.backward(torch.from_numpy(c.go).cuda())
    direct = launch("fp32", c.qkv, c.go, 0.125)
    assert bitwise_equal((out.detach().cpu(), x.grad.cpu()), (direct[0], direct[2]))
    assert_inside_bars(c, (out.detach().cpu(), direct[1], x.grad.cpu()), "functional.attention peaked T=129")


# ---------------------------------------------------------------- T sweep (bf16)
@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("T", EDGES)
def test_bf16_every_tile_edge(T, tiling):
    c = case("gauss", T)
    if T == 1:
        got = launch("bf16", c.qkv, c.go, 0.125, tiling)
        bf16_inside_bars(got, c.qkv, c.go, 0.125, (T, tiling))
        assert_inside_bf16_bars(case_bf16("gauss", T), got, f"edge gauss T={T} tiling={tiling}")
    else:
        check_against_rounded(c.qkv, c.go, 0.125, tiling)


# ---------------------------------------------------------------- structure (both families)
@pytest.mark.parametrize("tiling", EXPLICIT)
@pytest.mark.parametrize("T", [33, 129])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_slices_are_independent_bitwise(prec, T, tiling):
    """Slice (b, h) of a (2, T, 3 heads) launch equals the (1, T, 1 head) launch of that slice bit for bit: the same tiling is the same
    arithmetic, so any difference is an indexing leak between batches or heads."""
    c = case("peaked", T)
    out, lse, gq = launch(prec, c.qkv, c.go, 0.125, tiling)
    for b in range(B):
        for h in range(H):
            one = launch(prec, np.ascontiguousarray(c.qkv[b:b + 1, :, :, h:h + 1]), np.ascontiguousarray(c.go[b:b + 1, :, 64 * h:64 * h + 64]),
                         0.125, tiling)
            assert bitwise_equal(one, (out[b:b + 1, :, 64 * h:64 * h + 64], lse[b:b + 1, h:h + 1], gq[b:b + 1, :, :, h:h + 1])), (b, h)


# wave-tiles = ceil(T / 32) * H * B against the 1024 SIMDs: <= 256 one wave per group, <= 512 two, above four (attn_config).
# (B, T, H), the forward's tiling, the backward's.  The arithmetic of a query depends on the split alone (the waves of a block only
# share staged tiles), and with fewer key tiles than groups every split sums the same way: the first four shapes sit exactly on the
# thresholds, the last four have the same wave-tile counts with enough tiles (8, 257, 8, 3) for another split to give other bits.
AUTO = [((16, 33, 8), (1, 8), (1, 4)),       # 256
        ((257, 1, 1), (2, 4), (2, 4)),       # 257
        ((16, 33, 16), (2, 4), (2, 4)),      # 512
        ((19, 1, 27), (4, 2), (4, 2)),       # 513
        ((4, 250, 8), (1, 8), (1, 4)),       # 256
        ((1, 8200, 1), (2, 4), (2, 4)),      # 257
        ((8, 250, 8), (2, 4), (2, 4)),       # 512
        ((9, 70, 19), (4, 2), (4, 2))]       # 513


@pytest.mark.parametrize("shape,fwd,bwd", AUTO)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_automatic_choice_is_the_documented_tiling(prec, shape, fwd, bwd):
    b, T, h = shape
    assert -(-T // 32) * h * b in (256, 257, 512, 513)
    qkv, go = R.make_inputs("gauss", b, T, h)
    auto = launch(prec, qkv, go, 0.125)
    assert bitwise_equal(auto, launch(prec, qkv, go, 0.125, fwd, bwd))
    if T >= 70:     # another split is another order of the same sums: other bits, forward and (from the same out and lse) backward
        for other in EXPLICIT:
            if other[1] != fwd[1]:
                assert not bitwise_equal(auto[:2], launch(prec, qkv, go, 0.125, other, bwd)[:2]), other
            if other[1] != bwd[1]:
                assert not bitwise_equal(auto[2:], launch(prec, qkv, go, 0.125, fwd, other)[2:]), other


@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("T", [1, 33, 70])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_guard_bands(prec, T, tiling):
    """qkv, grad_out (NaN on both sides) and out, lse, grad_qkv (a sentinel on both sides) as views inside larger allocations: a read
    outside an operand poisons the result, a write outside an output changes a band.  Every access stays inside an allocation."""
    c = case("gauss", T, 0.125, 1, H)
    got, intact = launch(prec, c.qkv, c.go, 0.125, tiling, banded=True)
    assert intact, "a guard band of an output was written"
    if prec == "fp32":
        assert_inside_bars(c, got, f"banded T={T} tiling={tiling}")
    else:
        bf16_inside_bars(got, c.qkv, c.go, 0.125, (T, tiling))
        assert_inside_bf16_bars(case_bf16("gauss", T, 0.125, 1, H), got, f"banded T={T} tiling={tiling}")      # the same inputs as c
    assert bitwise_equal(got, launch(prec, c.qkv, c.go, 0.125, tiling))


@pytest.mark.parametrize("tiling", [(0, 0), (1, 8)])
def test_fp32_deterministic_run_to_run(tiling):
    qkv, go = R.make_inputs("gauss", 2, 578, 4)
    assert bitwise_equal(launch("fp32", qkv, go, 0.125, tiling), launch("fp32", qkv, go, 0.125, tiling))
