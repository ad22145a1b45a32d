"""The edge cases of the dense GEMM families (tests/dense_edges.py) without a GPU: the library's tile query returns the tile and the
split count every case claims, in both families; the lists together reach every tile, every split count, every listed row and column
tail; and each gate, applied to a CPU emulation of the family's contract, passes the emulation and rejects every planted fault
(a) .. (h) of dense_edges.mutants -- shown here, not assumed."""
import pytest
import torch

from tests import dense_edges as E
from tests import split_ref as R

U = E.U
EPS = 1e-5


def _query(ftx_lib, family, form, m, n, k):
    from fusiontransformer_amd import functional as spf
    return spf.dense_tile(family, form, m, n, k)


# ---------------------------------------------------------------- the case lists against the library's host query
@pytest.mark.parametrize("family", E.FAMILIES)
def test_checked_shapes_and_mirror(ftx_lib, family):
    for (m, n), (tile, rt, ct) in E.CHECKED_SHAPES.items():
        assert E.gemm_tile(m, n) == tile and E.tails(m, n, tile) == (rt, ct), (m, n)
        assert _query(ftx_lib, family, 0, m, n, 64) == tile + (1,), (m, n)
        assert (m, n, 64, tile, rt, ct) in E.GEMM_CASES
    for m, (splits, last) in E.WGRAD_ROWS.items():
        for n, k in E.WGRAD_NK + E.WGRAD_NK_MORE:
            assert E.wgrad_splits(m, n, k)[0::2] == (splits, last), (m, n, k)


@pytest.mark.parametrize("family", E.FAMILIES)
def test_gemm_cases_match_the_tile_query(ftx_lib, family):
    assert len(set(E.GEMM_CASES)) == len(E.GEMM_CASES)
    for m, n, k, tile, rt, ct in E.GEMM_CASES:
        assert k % 64 == 0 and n % 4 == 0 and m <= 2100 and n <= 2100 and k <= 192, (m, n, k)
        assert _query(ftx_lib, family, 0, m, n, k) == tile + (1,), (m, n, k)
        assert E.gemm_tile(m, n) == tile and E.tails(m, n, tile) == (rt, ct), (m, n, k)
        assert 1 <= rt <= tile[0] and 0 <= ct < tile[1] and (m - rt) % tile[0] == 0


@pytest.mark.parametrize("family", E.FAMILIES)
def test_wgrad_cases_match_the_tile_query(ftx_lib, family):
    assert len(set(E.WGRAD_CASES)) == len(E.WGRAD_CASES)
    ws_bytes = getattr(ftx_lib, f"ftx_dense_wgrad_{family}_workspace_bytes")
    for m, n, k, splits, last in E.WGRAD_CASES:
        assert n % 4 == 0 and k % 4 == 0, (m, n, k)
        assert _query(ftx_lib, family, 1, m, n, k) == (128, 128, splits), (m, n, k)
        s, length, rows = E.wgrad_splits(m, n, k)
        assert (s, rows) == (splits, last) and length % 64 == 0 and (splits - 1) * length + last == m, (m, n, k)
        assert ws_bytes(m, n, k) == (4 * splits * n * k if splits > 1 and 4 * splits * n * k > 256 else 256), (m, n, k)


@pytest.mark.parametrize("family", E.FAMILIES)
def test_form_cases_match_the_tile_query(ftx_lib, family):
    k = E.PATCH_C * E.PATCH_P ** 2
    assert k == 64
    for b, side, dim, t0, tile, rt in E.PATCH_CASES:
        g = (side // E.PATCH_P) ** 2
        assert g == 625 and g % 64 and t0 in (1, 2) and dim % 4 == 0
        assert _query(ftx_lib, family, 0, b * g, dim, k) == tile + (1,), (b, dim)
        assert E.tails(b * g, dim, tile)[0] == rt and rt < tile[0], (b, dim)
        assert b == 1 or any((f * g) % tile[0] for f in range(1, b)), "a frame border inside a tile"
    for b, g, t0, co, tile, rt in E.TAP_CASES:
        assert t0 in (0, 1, 2) and co in (4, 68, 96, 132)
        assert _query(ftx_lib, family, 0, b * g, co, E.TAP_DIM) == tile + (1,), (b, g, co)
        assert E.tails(b * g, co, tile)[0] == rt and rt < tile[0], (b, g, co)


def test_the_lists_reach_every_tile_split_and_tail():
    gemm = E.GEMM_CASES
    assert {c[3] for c in gemm} == set(E.TILES)
    for tile in E.TILES:
        mine = [c for c in gemm if c[3] == tile]
        assert {c[4] for c in mine if c[2] == 64} >= set(E.ROW_TAILS[tile]) | {tile[0]}, tile
        # a column tail at every tile: 4, and one that crosses a 32-column sub-tile; both with every listed row tail.  The plain
        # GEMM cases run in both weight orientations (tests/test_dense_edges_gpu.py), so this holds for w_kn = 0 and 1.
        for rt in E.ROW_TAILS[tile]:
            cts = {c[5] for c in mine if c[4] == rt and c[2] == 64}
            assert 4 in cts and cts & {36, 68}, (tile, rt)
        assert {c[5] for c in mine} >= ({0, 4, 36} if tile[1] == 64 else {0, 4, 36, 68}), tile
        assert {c[2] for c in mine} == {64, 128, 192}, tile
    wg = E.WGRAD_CASES
    assert {c[3] for c in wg} == set(range(1, 9))
    assert {c[4] for c in wg if c[3] > 1} >= {1, 2, 34, 65, 129, 193, 256}
    assert any(c[3] == 8 and c[4] == 1 for c in wg) and any(c[3] > 1 and c[4] % 2 == 1 and c[4] > 1 for c in wg)
    assert {c[1] for c in wg} == {4, 68, 132, 260} and {c[2] for c in wg} == {4, 68, 132, 260}
    assert any(c[1] % 128 and c[3] > 1 for c in wg) and any(c[2] % 128 and c[3] > 1 for c in wg), "n and k tails with several splits"
    assert any(c[1] == 132 and c[2] == 132 for c in wg), "two tiles per side"
    assert {c[4] for c in E.PATCH_CASES} == set(E.TILES) and {c[3] for c in E.PATCH_CASES} == {1, 2}
    assert {c[2] for c in E.PATCH_CASES} == {768, 772}
    for tile in E.TILES:
        assert {c[2] for c in E.PATCH_CASES if c[4] == tile} == {768, 772}, "a column tail at every tile"
    assert {c[4] for c in E.TAP_CASES} == set(E.TILES)
    assert {c[2] for c in E.TAP_CASES} == {0, 1, 2} and {c[3] for c in E.TAP_CASES} == {4, 68, 96, 132}


def test_g2_from_parts_is_split_refs_g2():
    x, w, b = E.data(70, 64, 68, 1)
    out = R.gemm(x, w.t(), R.SIX, accumulate="fp32") + b
    assert E.g2_figures(out, E.g2_parts(x, w.t()), b) == R.g2_figures(out, x, w.t(), b)


# ---------------------------------------------------------------- the gates tell, on an emulation of the contract
def _gate(family, out, ref, bound, faults, what):
    print(f"{what} {family}: emulation at {E.worst(out, ref, bound):.3g} of the bound; faults at "
          + ", ".join(f"({n}) {E.worst(out, r, bound):.3g}" for n, r in sorted(faults.items())))
    assert E.passes(out, ref, bound), (what, family, E.worst(out, ref, bound))
    for name, r in faults.items():
        assert not E.passes(out, r, bound), (what, family, name)


@pytest.mark.parametrize("family", E.FAMILIES)
def test_gates_pass_the_emulated_gemm_and_reject_c_d_e_f(family):
    m, n, k = 97, 100, 64
    assert (m, n, k, (64, 64), 33, 36) in E.GEMM_CASES
    x, w, b = E.data(m, k, n, seed=m + n)
    b_kn = w.t().contiguous()
    s, sa = E.gemm_ref(family, x, b_kn)
    f = E.factor(family, k)
    a64, b64 = E.operands64(family, x, b_kn)
    # forward: BIAS, and the GELU behind it
    pre = (E.emulate(family, x, b_kn) + b.double()).float()
    pre_ref, pre_bound = E.bias_ref(s, sa, b, f)
    faults = E.mutants("gemm", a=a64, b_kn=b64, bias=b.double(), col_tail=36)
    assert sorted(faults) == ["c", "d", "f"]
    _gate(family, pre, pre_ref, pre_bound, faults, "BIAS")
    h = E._gelu64(pre.double()).float()
    h_ref, h_bound = E.gelu_ref(pre_ref, pre_bound, pre)
    _gate(family, h, h_ref, h_bound, {n: E._gelu64(r) for n, r in faults.items()}, "BIAS_GELU")
    # data gradient: W stored [K][N], NONE and DGELU
    out = E.emulate(family, x, b_kn).float()
    faults = E.mutants("dx", a=a64, b_kn=b64)
    assert sorted(faults) == ["c", "d", "e"]
    _gate(family, out, s, f * U * sa, faults, "dX NONE")
    p = E.randn((m, n), 5, scale=2.0)
    d_ref, d_bound = E.dgelu_ref(s, sa, p, f)
    d64 = E._dgelu64(p.double())
    _gate(family, (out.double() * d64).float(), d_ref, d_bound, {n: r * d64 for n, r in faults.items()}, "dX DGELU")
    if family == "split":
        e, t = E.g2_figures(pre, E.g2_parts(x, b_kn), b)
        assert out.numel() >= E.G2_MIN_ELEMS and e <= t / 2, (e, t)
        for name, r in faults.items():
            e, t = E.g2_figures(r.float(), E.g2_parts(x, b_kn))
            assert e > t / 2, name


@pytest.mark.parametrize("m", [513, 2241])
@pytest.mark.parametrize("family", E.FAMILIES)
def test_gates_pass_the_emulated_wgrad_and_reject_a_b(family, m):
    n = k = 68
    splits, length, last = E.wgrad_splits(m, n, k)
    assert (m, n, k, splits, last) in E.WGRAD_CASES and splits > 1
    dy, x = E.randn((m, n), m, scale=0.1), E.randn((m, k), m + 1)
    gt = dy.t().contiguous()
    s, sa = E.gemm_ref(family, gt, x)
    g64, x64 = E.operands64(family, dy, x)
    faults = E.mutants("wgrad", g=g64, x=x64, split_len=length)
    assert sorted(faults) == ["a", "b"]
    _gate(family, E.emulate(family, gt, x).float(), s, E.wgrad_factor(family, m, splits) * U * sa, faults, f"dW m={m}")


@pytest.mark.parametrize("family", E.FAMILIES)
def test_gates_pass_the_emulated_forms_and_reject_g_h(family):
    # patch embedding
    b, side, dim, t0, tile, rt = E.PATCH_CASES[3]
    assert b >= 2
    g = (side // E.PATCH_P) ** 2
    img = E.randn((b, E.PATCH_C, side, side), 1)
    w, bias, pos = E.randn((dim, 64), 2, scale=0.02), E.randn((dim,), 3, scale=0.1), E.randn((t0 + g, dim), 4, scale=0.02)
    ref, bound, a, add = E.patch_ref(family, img, w, bias, pos, t0, E.factor(family, 64))
    a64, w64 = E.operands64(family, a, w.t())
    faults = E.mutants("patch", a=a64, b_kn=w64, bias=bias.double(), pos=pos.double(), g=g, t0=t0)
    faults.update({n: r + add for n, r in E.mutants("dx", a=a64, b_kn=w64).items() if n in "cd"})
    assert sorted(faults) == ["c", "d", "g"]
    _gate(family, (E.emulate(family, a, w.t()) + add).float(), ref, bound, faults, "patch embed")
    # tap stem
    b, g, t0, co, tile, rt = E.TAP_CASES[1]
    assert t0 >= 1
    tokens = E.randn((b, t0 + g, E.TAP_DIM), 5)
    w, bias = E.randn((co, E.TAP_DIM), 6, scale=0.05), E.randn((co,), 7, scale=0.5)
    gamma, beta = torch.rand(co, generator=torch.Generator().manual_seed(8)) + 0.5, E.randn((co,), 9, scale=0.2)
    mean, var = E.randn((co,), 10, scale=0.3), torch.rand(co, generator=torch.Generator().manual_seed(11)) + 0.5
    bn = (gamma, beta, mean, var, EPS)
    f = E.factor(family, E.TAP_DIM)
    ref, bound = E.tap_ref(family, tokens, w, bias, *bn, t0, f)
    faults = E.mutants("tap", ref_unskipped=E.tap_ref(family, tokens, w, bias, *bn, t0, f, skip=False)[0])
    a = tokens[:, t0:].reshape(b * g, E.TAP_DIM)
    pre = (E.emulate(family, a, w.t()) + bias.double()).float()
    out = E.bn64(pre.double().clamp_min(0), *bn).float()
    _gate(family, out, ref, bound, faults, "tap stem")
