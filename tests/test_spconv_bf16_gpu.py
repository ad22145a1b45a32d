"""bf16-operand sparse convolution (csrc/ftx_spconv_bf16.hip, bf16=True in functional) against its precision contract.

The reference is float64 applied to the bf16-ROUNDED operands (t.to(torch.bfloat16).double()).  A bf16 x bf16 product is exact in
fp32, so the only error left is the fp32 accumulation, and every element is gated as in tests/test_spconv_regimes_gpu.py:

    |got - ref| <= (m + 8) * 2^-24 * R

with R the same computation on |rounded operands| and m the kernel's chain: c_in + kvol for pair GEMM + reduce and the scatter form,
c_in (+ 1 with a bias) for dense rows, tile length + tiles of the offset + 16 for the weight gradient.  The gate must be able to fail:
it rejects the float64 result of the UNROUNDED operands (so the operands really are rounded) and the two mutants of the regime tests
(one pair removed, one pair moved to the neighbouring offset).

Layers come from tests/spconv_regimes.py (the benched batch at full size)."""
import numpy as np
import pytest
import torch

from tests import spconv_regimes as S
from tests.helpers import oracle_inputs, product_inputs, small_cfg
from tests.test_spconv_regimes_gpu import (U, WORST, bench_maps, check, conv_mutants, conv_ref, gen, get_map, pair_list, randn,  # noqa: F401
                                           random_sizes, ratio, wgrad_mutants, wgrad_ref, WGRAD_CASES, GEMM_CASES)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield spf, _lib.load()
    print("\nbf16: worst error / bound per kernel: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items()) if k.endswith("bf16")))


def bf(t):
    """t rounded to bf16 (round-to-nearest-even), as float64."""
    return t.to(torch.bfloat16).double()


def wgrad_bf16_tile_len(lib, n_pairs, ca, cg, kvol):
    """csrc/ftx_spconv_common.h spconv_wgrad_tile_len<SpconvBf16>() (table and step: csrc/ftx_spconv_bf16.hip), checked against the library's
    workspace query."""
    mi, wmg, ni, wng = S.wgrad_config(ca, cg)
    mn_tiles = S.cdiv(ca, 32 * mi * wmg) * S.cdiv(cg, 32 * ni * wng)
    slots = 256 * int(lib.ftx_spconv_wgrad_bf16_table_blocks(mi, wmg, ni, wng))
    length = 256
    for rounds in range(1, 65):
        tiles = max((slots * rounds * 15 // 16) // mn_tiles - (kvol + 1) // 2, 1)
        length = S.cdiv(S.cdiv(n_pairs, tiles), 128) * 128
        if length <= 4096:
            break
    length = max(length, 256)
    tiles = int(lib.ftx_spconv_pairs_wgrad_bf16_workspace_bytes(n_pairs, ca, cg, kvol)) // (4 * ca * cg)
    assert tiles == S.cdiv(n_pairs, length) + kvol, (n_pairs, ca, cg, kvol, tiles, length)
    return length


def conv_check_bf16(kernel, what, got, A, W, src, dst, koff, n_dst, unrounded=True):
    """Pair GEMM (+ reduce) on rounded operands: the gate, its two mutants, and (unrounded=True) the rejection of the float64 result
    of the unrounded operands."""
    Ar, Wr = bf(A), bf(W)
    ref = conv_ref(Ar, Wr, src, dst, koff, n_dst)
    bound = (W.shape[1] + W.shape[0] + 8) * U * conv_ref(Ar.abs(), Wr.abs(), src, dst, koff, n_dst)
    check(kernel, what, got, ref, bound, conv_mutants(Ar, Wr, src, dst, koff))
    if unrounded:
        exact = conv_ref(A.double(), W.double(), src, dst, koff, n_dst)
        assert ratio(exact, ref, bound) > 1.0, f"{what}: the gate accepts the unrounded operands"
    return ref


def wgrad_check_bf16(lib, what, got, A, ia, G, ig, koff, unrounded=True):
    Ar, Gr = bf(A), bf(G)
    ref = wgrad_ref(Ar, ia, Gr, ig, koff)
    kvol, n = koff.shape[0] - 1, int(koff[-1])
    length = wgrad_bf16_tile_len(lib, n, A.shape[1], G.shape[1], kvol)
    tiles = (koff[1:] - koff[:-1] + length - 1) // length
    m = (length + tiles + 16).double().view(kvol, 1, 1)
    bound = (m + 8) * U * wgrad_ref(Ar.abs(), ia, Gr.abs(), ig, koff)
    check("pairs_wgrad_bf16", what, got, ref, bound, wgrad_mutants(Ar, ia, Gr, ig, koff))
    if unrounded:
        exact = wgrad_ref(A.double(), ia, G.double(), ig, koff)
        assert ratio(exact, ref, bound) > 1.0, f"{what}: the gate accepts the unrounded operands"
    return ref


# ---------------------------------------------------------------- production layers at full size
@pytest.mark.parametrize("e", S.PRODUCTION, ids=[e["name"] for e in S.PRODUCTION])
def test_production_layer_bf16(env, bench_maps, e):
    spf, L = env
    km = get_map(bench_maps, e["map"])
    assert km.n_pairs == e["n_pairs"], (e["name"], km.n_pairs)
    kvol, ca, co, P = km.kvol, e["ca"], e["co"], km.n_pairs
    if e["form"] == "deconv":
        src_d, dst_d, n_src, n_dst, pos_f, pos_b = km.pair_out, km.pair_in, km.n_out, km.n_in, None, km.pos
    else:
        src_d, dst_d, n_src, n_dst, pos_f, pos_b = km.pair_in, km.pair_out, km.n_in, km.n_out, km.pos, (None if e["form"] == "down_dgrad" else km.pos_t)
    src, dst, koff = src_d.long().cpu(), dst_d.long().cpu(), km.koff.long().cpu()
    g = gen(len(e["name"]) + ca + co + 1)
    A, W, G = randn(g, n_src, ca), randn(g, kvol, ca, co, scale=(ca * kvol) ** -0.5), randn(g, n_dst, co)
    Ad, Wd, Gd = A.cuda(), W.cuda(), G.cuda()

    assert L.ftx_spconv_gemm_bf16_block_cols(co, P, kvol) == e["fwd"] and L.ftx_spconv_gemm_bf16_block_cols(ca, P, kvol) == e["dgrad"]
    if pos_f is None:
        out = spf._spconv_direct(Ad, Wd, src_d, dst_d, km.koff, P, n_dst, co, 0, bf16=True)
        conv_check_bf16("pairs_gemm_scatter_bf16", e["name"] + " forward", out, A, W, src, dst, koff, n_dst)
    else:
        out = spf._spconv_apply(Ad, Wd, src_d, pos_f, km.koff, P, n_dst, co, 0, bf16=True)
        conv_check_bf16("pairs_gemm+reduce_bf16", e["name"] + " forward", out, A, W, src, dst, koff, n_dst)
    Wt = W.transpose(1, 2)
    if pos_b is None:
        gin = spf._spconv_direct(Gd, Wd, dst_d, src_d, km.koff, P, n_src, ca, 1, bf16=True)
        conv_check_bf16("pairs_gemm_scatter_bf16", e["name"] + " data gradient", gin, G, Wt, dst, src, koff, n_src)
    else:
        gin = spf._spconv_apply(Gd, Wd, dst_d, pos_b, km.koff, P, n_src, ca, 1, bf16=True)
        conv_check_bf16("pairs_gemm+reduce_bf16", e["name"] + " data gradient", gin, G, Wt, dst, src, koff, n_src)
    dW = spf._spconv_wgrad(Ad, src_d, Gd, dst_d, km.koff, P, bf16=True)
    wgrad_check_bf16(L, e["name"] + " weight gradient", dW, A, src, G, dst, koff)
    # deterministic: a second launch of each gives the same bits
    assert torch.equal(spf._spconv_wgrad(Ad, src_d, Gd, dst_d, km.koff, P, bf16=True), dW)
    if pos_f is not None:
        assert torch.equal(spf._spconv_apply(Ad, Wd, src_d, pos_f, km.koff, P, n_dst, co, 0, bf16=True), out)


@pytest.mark.parametrize("e", S.DENSE, ids=[e["name"] for e in S.DENSE])
def test_dense_rows_bf16_with_and_without_bias(env, e):
    """functional.linear(bf16=True) (bias) and rows_matmul(bf16=True) (no bias) on 81 k rows: outputs, input gradients, dense-mode
    weight gradients."""
    spf, L = env
    n, ca, co = e["rows"], e["ca"], e["co"]
    g = gen(ca * 1000 + co + 1)
    x, W, b, go = randn(g, n, ca), randn(g, co, ca, scale=ca ** -0.5), randn(g, co), randn(g, n, co)
    assert L.ftx_spconv_gemm_bf16_block_cols(co, n, 0) == e["fwd"] and L.ftx_spconv_gemm_bf16_block_cols(ca, n, 0) == e["dgrad"]
    r, c, j = n // 2, ca // 2, co // 2
    xr, Wr, gr, b64 = bf(x), bf(W), bf(go), b.double()
    for bias in (True, False):
        a_c, g_c = (co, ca) if bias else (ca, co)     # linear: dW = go^T x; rows_matmul: dK = x^T go
        length = wgrad_bf16_tile_len(L, n, a_c, g_c, 1)
        m_w = length + S.cdiv(n, length) + 16
        xd, Wd = x.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
        bd = b.cuda().requires_grad_(True) if bias else None
        if bias:
            y = spf.linear(xd, Wd, bd, bf16=True)
        else:
            y = spf.rows_matmul(xd, Wd.t().contiguous(), bf16=True)   # kernel (ca, co)
        y.backward(go.cuda())
        tag = e["name"] + (" linear" if bias else " matmul")
        ref = xr @ Wr.T + (b64 if bias else 0)
        bound = (ca + int(bias) + 8) * U * (xr.abs() @ Wr.abs().T + (b64.abs() if bias else 0))
        check("rows_gemm_bf16", tag + " forward", y, ref, bound,
              [[((r,), -xr[r, c] * Wr[:, c])], [((r,), xr[r, c] * (Wr[:, c + 1] - Wr[:, c]))]])
        assert ratio(x.double() @ W.double().T + (b64 if bias else 0), ref, bound) > 1.0, "the gate accepts the unrounded operands"
        ref = gr @ Wr
        bound = (co + 8) * U * (gr.abs() @ Wr.abs())
        check("rows_gemm_bf16", tag + " input gradient", xd.grad, ref, bound,
              [[((r,), -gr[r, j] * Wr[j])], [((r,), gr[r, j] * (Wr[j + 1] - Wr[j]))]])
        ref = gr.T @ xr
        bound = (m_w + 8) * U * (gr.abs().T @ xr.abs())
        gw = Wd.grad
        check("pairs_wgrad_bf16", tag + " weight gradient", gw, ref, bound,
              [[((slice(None),), -torch.outer(gr[r], xr[r]))], [((slice(None),), torch.outer(gr[r], xr[r + 1] - xr[r]))]])


def test_library_fallback_rounds_the_same_way(env):
    """Shapes the tile kernel does not take (channels not a multiple of 4) go to a library GEMM on the same rounded operands."""
    spf, _ = env
    g = gen(77)
    x, W, b, go = randn(g, 3000, 30), randn(g, 18, 30, scale=30 ** -0.5), randn(g, 18), randn(g, 3000, 18)
    xd, Wd, bd = x.cuda().requires_grad_(True), W.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = spf.linear(xd, Wd, bd, bf16=True)
    y.backward(go.cuda())
    xr, Wr, gr = bf(x), bf(W), bf(go)
    for got, ref, m, R in ((y, xr @ Wr.T + b.double(), 31, xr.abs() @ Wr.abs().T + b.double().abs()), (xd.grad, gr @ Wr, 18, gr.abs() @ Wr.abs()),
                           (Wd.grad, gr.T @ xr, 3000, gr.abs().T @ xr.abs())):
        d = (got.detach().cpu().double() - ref).abs()
        assert bool((d <= (m + 8) * U * R + 1e-30).all()), float((d / (R * U)).max())


# ---------------------------------------------------------------- every instantiation, synthetic pair lists
@pytest.mark.parametrize("w_t", [0, 1])
@pytest.mark.parametrize("ca,co,n_pairs,cols", GEMM_CASES)
def test_pair_gemm_bf16_every_column_block(env, ca, co, n_pairs, cols, w_t):
    spf, L = env
    g = gen(ca * 7 + co * 13 + n_pairs + w_t + 1)
    sizes = random_sizes(g, n_pairs, 27)
    n_src, n_dst = 5000, max(sizes) + 17
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    assert L.ftx_spconv_gemm_bf16_block_cols(co, n_pairs, 27) == cols
    A = randn(g, n_src, ca)
    Wl = randn(g, 27, ca, co, scale=(ca * 27) ** -0.5)
    Ws = Wl.transpose(1, 2).contiguous() if w_t else Wl
    out = spf._spconv_apply(A.cuda(), Ws.cuda(), d["src"], d["pos"], d["koff"], n_pairs, n_dst, co, w_t, bf16=True)
    conv_check_bf16("pairs_gemm+reduce_bf16", f"{ca}->{co} wT={w_t}", out, A, Wl, src, dst, koff, n_dst)


@pytest.mark.parametrize("ca,cg,sides", WGRAD_CASES)
def test_wgrad_bf16_every_instantiation(env, ca, cg, sides):
    """Every reachable (MI, WMG) x (NI, WNG) pair of tile sides ((3,1) x (3,1) is sent to (2,2) x (3,1), as in fp32)."""
    spf, L = env
    assert S.wgrad_config(ca, cg) == (sides if sides != (3, 1, 3, 1) else (2, 2, 3, 1))
    g = gen(ca * 31 + cg + 1)
    sizes = random_sizes(g, 30000, 27)
    n_src, n_dst = 4000, max(sizes) + 5
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    A, G = randn(g, n_src, ca), randn(g, n_dst, cg)
    dW = spf._spconv_wgrad(A.cuda(), d["src"], G.cuda(), d["dst"], d["koff"], int(koff[-1]), bf16=True)
    wgrad_check_bf16(L, f"{ca}x{cg} {sides}", dW, A, src, G, dst, koff)


@pytest.mark.parametrize("kvol,ca,cg", [(27, 32, 32), (8, 128, 96), (5, 4, 64)])
def test_tile_edges_bf16(env, kvol, ca, cg):
    """Offset sizes around the 32-pair steps, the 128-pair GEMM tiles and the bf16 weight-gradient tile length L (L-1, L, L+1, many
    tiles), empty offsets; pair GEMM + reduce and weight gradient."""
    spf, L = env
    length = 256
    for _ in range(20):
        sizes = [v if isinstance(v, int) else (length if v == "L" else (int(v[:-1]) * length + 1 if v.endswith("L") else length + int(v[1:])))
                 for v in S.EDGE_SIZES[kvol]]
        new = wgrad_bf16_tile_len(L, sum(sizes), ca, cg, kvol)
        if new == length:
            break
        length = new
    g = gen(kvol * 100 + ca + cg)
    P = sum(sizes)
    n_src, n_dst = 3000, max(sizes) + 3
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    A, W, G = randn(g, n_src, ca), randn(g, kvol, ca, cg, scale=(ca * kvol) ** -0.5), randn(g, n_dst, cg)
    out = spf._spconv_apply(A.cuda(), W.cuda(), d["src"], d["pos"], d["koff"], P, n_dst, cg, 0, bf16=True)
    conv_check_bf16("pairs_gemm+reduce_bf16", f"edges kvol {kvol}", out, A, W, src, dst, koff, n_dst)
    dW = spf._spconv_wgrad(A.cuda(), d["src"], G.cuda(), d["dst"], d["koff"], P, bf16=True)
    wgrad_check_bf16(L, f"edges kvol {kvol}", dW, A, src, G, dst, koff)


def test_out_of_range_gather_gives_a_zero_row(env):
    """Source indices below 0 or past the last row give a zero pair row; every other row is the product of its gathered row."""
    spf, L = env
    g = gen(5)
    sizes = [300, 0, 517, 129]
    n_src, n_dst = 900, 600
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    bad = [3, 301, 700, 945]
    s = d["src"].clone()
    s[bad[0]], s[bad[1]], s[bad[2]], s[bad[3]] = -1, n_src, n_src + 1000, -7
    A, W = randn(g, n_src, 64), randn(g, 4, 64, 96, scale=0.1)
    Ad, Wd = A.cuda(), W.cuda()      # held until the launch has finished: the kernel reads them through raw pointers
    tmp = torch.full((sum(sizes), 96), float("nan"), device="cuda")
    spf.check(L.ftx_spconv_pairs_gemm_bf16(Ad.data_ptr(), n_src, s.data_ptr(), Wd.data_ptr(), 0, d["koff"].data_ptr(), sum(sizes), 64, 96,
                                           4, tmp.data_ptr(), spf._lib.stream()), "gemm")
    tmp = tmp.cpu()
    del Ad, Wd
    assert bool((tmp[bad] == 0).all())
    ok = torch.ones(sum(sizes), dtype=torch.bool)
    ok[bad] = False
    k_of = torch.repeat_interleave(torch.arange(4), torch.tensor(sizes))
    ref = torch.einsum("pc,pcd->pd", bf(A)[src[ok]], bf(W)[k_of[ok]])
    assert float((tmp[ok].double() - ref).abs().max()) <= 1e-4


def test_conv_bn_node_matches_sparse_conv_then_batch_norm(env, bench_maps):
    """The fused node (bf16=True) against sparse_conv(bf16=True) + batch_norm: the convolution output it keeps, its output and the
    gradients of input, weight, gamma and beta, bit for bit (reduce_stats sums the offsets in the reduce's order, and the BatchNorm
    statistics come out the same from either pass); and its own repeatability."""
    spf, L = env
    km = bench_maps.kernel_map(3, 4, 1)
    ca, co, kvol, n = 192, 128, 27, km.n_out
    g = gen(1920)
    A, W = randn(g, n, ca), randn(g, kvol, ca, co, scale=(ca * kvol) ** -0.5)
    gam, bet, gy = torch.rand(co, generator=g).float() + 0.5, randn(g, co), randn(g, n, co).cuda()

    def fused():
        Ad, Wd = A.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
        gd, bd = gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
        y = spf.conv_bn_train(Ad, Wd, km, False, gd, bd, torch.zeros(co, device="cuda"), torch.ones(co, device="cuda"), 0.1, 1e-5, relu=True, bf16=True)
        x = y.grad_fn.saved_tensors[2].detach().clone()
        y.backward(gy)
        return x, y.detach(), Ad.grad, Wd.grad, gd.grad, bd.grad

    Ad, Wd = A.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
    gd, bd = gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
    x2 = spf.sparse_conv(Ad, Wd, km, False, bf16=True)
    y2 = spf.batch_norm(x2, gd, bd, torch.zeros(co, device="cuda"), torch.ones(co, device="cuda"), True, 0.1, 1e-5, relu=True)
    y2.backward(gy)
    a, b = fused(), fused()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[0], x2.detach())
    for name, u, v in zip(("y", "gA", "gW", "ggamma", "gbeta"), a[1:], (y2.detach(), Ad.grad, Wd.grad, gd.grad, bd.grad)):
        assert torch.equal(u, v), name


# ---------------------------------------------------------------- model level
def _model(seed, lidar_bf16):
    from fusiontransformer_amd.models.build import build_model
    from oracle import ft_oracle as O
    cfg = small_cfg("middle")
    torch.manual_seed(seed)
    oracle = O.build_model(dict(cfg.MODEL))
    cfg.MODEL.lidar_bf16 = lidar_bf16
    model, _, _ = build_model(cfg)
    model.load_state_dict(oracle.state_dict())
    return cfg, oracle, model.cuda()


def _round_oracle_lidar(oracle, monkeypatch):
    """The oracle with every LiDAR-branch matmul operand rounded to bf16: sparse convolutions (sparseconv_op), the k = 1 convolutions,
    the point-transform and middle-fusion Linears.  The heads stay fp32."""
    import types
    from oracle import ft_oracle as O
    r = lambda t: t.to(torch.bfloat16).float()   # noqa: E731
    orig = O.sparseconv_op
    monkeypatch.setattr(O, "sparseconv_op", lambda feats, kernel, idx, n_out, t: orig(r(feats), r(kernel), idx, n_out, t))
    lb = oracle.lidar_backbone
    for m in lb.modules():
        if isinstance(m, O.Conv3d) and m.kernel_size == 1 and m.stride == 1:
            def fwd(self, x):
                out = O.SparseTensor(r(x.F) @ r(self.kernel), x.C, x.s)
                out.coord_maps, out.kernel_maps = x.coord_maps, x.kernel_maps
                return out
            m.forward = types.MethodType(fwd, m)
    lins = [seq[0] for seq in lb.point_transforms] + [lb.middle_fusion_transform[0]]
    for lin in lins:
        lin.forward = types.MethodType(lambda self, x: torch.nn.functional.linear(r(x), r(self.weight), self.bias), lin)
    return len(lins)


def test_lidar_bf16_model_matches_the_rounded_oracle(monkeypatch):
    """Middle fusion, small frames, eval: lidar_bf16=True against the CPU oracle whose LiDAR-branch GEMM operands are rounded to bf16.
    Agreement within 2e-3 max-abs on the LiDAR logits (the fp32 path is held to 1e-3 against the plain oracle); the RMS distance from
    the plain oracle is at least 10x the RMS distance from the rounded one, so the mode is engaged.  The image branch is fp32 in both.
    Measured on an MI355X: vs the rounded oracle max 1.3e-4, RMS 6.2e-6; vs the plain oracle max 7.0e-4, RMS 7.3e-5 (11.9x).  The max
    ratio is only ~5x: where an operand sits next to a bf16 rounding boundary, a last-bit difference of the fp32 sums ahead of it moves
    it by one bf16 step, which a few logits show; RMS sees the systematic effect of the rounding."""
    from fusiontransformer_amd.data.synth import make_batch
    cfg, oracle, model = _model(3, True)
    batch = make_batch([0, 1], max_points=2500)
    oracle.eval(); model.eval()
    with torch.no_grad():
        out = model(product_inputs(batch))
        plain = oracle(oracle_inputs(batch))
        assert _round_oracle_lidar(oracle, monkeypatch) == 4
        rounded = oracle(oracle_inputs(batch))
    keys = ("lidar_seg_logit", "lidar_seg_logit2")
    err_r = max((out[k].cpu() - rounded[k]).abs().max().item() for k in keys)
    err_p = max((out[k].cpu() - plain[k]).abs().max().item() for k in keys)
    rms = lambda a, b: max(float((a[k].cpu() - b[k]).double().pow(2).mean().sqrt()) for k in keys)   # noqa: E731
    rms_r, rms_p = rms(out, rounded), rms(out, plain)
    err_img = max((out[k].cpu() - plain[k]).abs().max().item() for k in ("img_seg_logit", "img_seg_logit2"))
    print(f"\nlidar_bf16 logits: vs rounded oracle max {err_r:.3g} rms {rms_r:.3g}, vs plain oracle max {err_p:.3g} rms {rms_p:.3g}; "
          f"image logits vs oracle {err_img:.3g}")
    assert err_r <= 2e-3, err_r
    assert rms_p >= 10 * rms_r, (rms_p, rms_r)
    assert err_img <= 1e-3, err_img


def _step_log(model, pin):
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.trainer import fusion_losses
    model.image_backbone.backbone.use_graphs = False
    model.train()
    spf.LAUNCH_LOG = []
    try:
        out = model(pin)
        l2, l3 = fusion_losses(out, pin["seg_label"], None, 0.1, True)
        (l2 + l3).backward()
        torch.cuda.synchronize()
        return [k for k, *_ in spf.LAUNCH_LOG]
    finally:
        spf.LAUNCH_LOG = None


def test_launch_kinds_follow_the_switch():
    from fusiontransformer_amd.data.synth import make_batch
    pin = product_inputs(make_batch([0], max_points=1500))
    kinds = _step_log(_model(4, False)[2], pin)
    assert "spconv_pairs_gemm" in kinds and not any(k.endswith("_bf16") for k in kinds), sorted(set(kinds))
    kinds = _step_log(_model(4, True)[2], pin)
    sp = {k for k in kinds if k.startswith("spconv_")}
    assert sp == {"spconv_pairs_gemm_bf16", "spconv_pairs_wgrad_bf16", "spconv_reduce"}, sp


def test_lidar_bf16_graphed_two_stream_step_is_bit_identical_to_eager_twin():
    """With lidar_bf16=True, a training step with the graphed trunk on two streams against an eager-trunk, one-stream twin: logits
    and every gradient bit for bit (capturing step and a replay)."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.trainer import fusion_losses
    pin = product_inputs(make_batch([2, 3], max_points=3000))

    def run(graphs, steps):
        cfg, oracle, model = _model(5, True)
        model.train()
        vit = model.image_backbone.backbone
        vit.use_graphs = graphs
        model.overlap_branches = graphs
        res = []
        for _ in range(steps):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(0)
            out = model(pin)
            l2, l3 = fusion_losses(out, pin["seg_label"], None, 0.1, True)
            (l2 + l3).backward()
            torch.cuda.synchronize()
            res.append(({k: v.detach().clone() for k, v in out.items()}, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
        if graphs:
            assert vit.__dict__.get("_graph_cache") and all(v is not None for v in vit._graph_cache.values()), "the trunk was not captured"
        return res

    graphed = run(True, 2)
    eager = run(False, 1)[0]
    for outs, grads in graphed:
        for k in eager[0]:
            assert torch.equal(outs[k], eager[0][k]), k
        assert grads.keys() == eager[1].keys()
        for n in grads:
            assert torch.equal(grads[n], eager[1][n]), n
