"""Three-piece split sparse convolution (csrc/ftx_spconv_split.hip, operands="split" in functional, cfg.MODEL.lidar_split) against
its precision contract: fp32-class results from the bf16 MFMA.

Both gates compare with float64 on the UNROUNDED operands (tests/spconv_split_ref.py derives them):

    G1, per element:  |got - S| <= (6 m_g + m_r + 8) * 2^-24 * R        G2:  rms(got - S) <= rms(S5 - S) / 2

m_g = c_in for the pair GEMM, the scatter form and dense rows, tile length + tiles of the offset + 16 for the weight gradient (this
family's tile length, checked against its workspace query); m_r = kvol for the reduce over the offsets (0 for the scatter form, which
has none), + 1 with a bias.  G2 is
asserted from 4 096 output elements on.  Every value test also asserts that the gate rejects the two mutants of the regime tests (one
pair removed, one pair moved to the neighbouring offset), that the gates reject the bf16 family's result on the same operands (so the
split is really engaged; G1 where it can, else G2), and that a second launch returns the same bits.  At full size the weight-gradient mutants are planted in the pair
the derived bound resolves best (tests/spconv_split_ref.py wgrad_mutants_resolved says why the middle of an 81 k-pair offset is not it).  Next to each split result the fp32 family runs on the same
operands; the module prints the worst error of both in units of 2^-24 R.

Layers come from tests/spconv_regimes.py (the benched batch at full size: the pair GEMM under G1 only there, the float64 piece
references of its G2 are too slow at that size; the weight gradient, whose result is one small matrix per offset, under both)."""
import pytest
import torch

from tests import spconv_regimes as S
from tests import spconv_split_ref as SR
from tests import split_ref as R
from tests.helpers import oracle_inputs, product_inputs, small_cfg
from tests.test_spconv_regimes_gpu import (U, WORST, bench_maps, check, conv_mutants, gen, get_map, pair_list, randn,  # noqa: F401
                                           random_sizes, ratio, wgrad_mutants, WGRAD_CASES, GEMM_CASES)

pytestmark = pytest.mark.gpu
UNITS = {}      # kernel -> worst |error| / (2^-24 R) on the operands of this module, split and fp32 side by side


@pytest.fixture(scope="module")
def env():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield spf, _lib.load()
    print("\nsplit: worst error / bound per kernel: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items()) if k.endswith("_split")))
    print("worst error in units of 2^-24 R, same operands: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(UNITS.items())))


def units(kernel, got, ref, bound, m):
    """Records max |got - ref| / (2^-24 R) for `kernel`, from the bound = m * 2^-24 * R."""
    UNITS[kernel] = max(UNITS.get(kernel, 0.0), ratio(got.detach().cpu(), ref, bound / m))


def gate(kernel, what, got, ref, bound, m, mutants, bf16_got, fp32_got=None, s5=None):
    """G1 with its two mutants, G2 where S5 is given, the rejection of the bf16 family's result by G1 or G2, and the figures.
    (G1 is a worst-case bound, linear in the chain; the error of rounded operands on random data grows with its square root.  The
    pair GEMM's chains are c_in <= 384 and G1 alone rejects the bf16 result there; a weight gradient over tens of thousands of pairs per
    offset needs G2 for that, so the weight-gradient checks always bring S5.)"""
    check(kernel, what, got, ref, bound, mutants)
    units(kernel, got, ref, bound, m)
    if fp32_got is not None:
        units(kernel.replace("_split", "_fp32"), fp32_got, ref, bound, m)
    rejected = ratio(bf16_got.detach().cpu(), ref, bound) > 1.0 or (s5 is not None and not SR.g2_passes(bf16_got, ref, s5))
    assert rejected, f"{what}: the gates accept the bf16 family's result"
    if s5 is not None and ref.numel() >= SR.G2_MIN_ELEMENTS:
        e, t = SR.g2_figures(got, ref, s5)
        print(f"\n{what}: G2 E / T = {e / t:.3g}")
        assert e <= t / 2, f"{what}: G2 E = {e:.3g}, T = {t:.3g}"


def conv_check_split(kernel, what, got, A, W, src, dst, koff, n_dst, bf16_got, fp32_got=None, g2=True):
    m_r = 0 if "scatter" in kernel else W.shape[0]      # the scatter form writes each row once: no reduce over the offsets
    ref, bound = SR.conv_gate(A, W, src, dst, koff, n_dst, reduce_chain=m_r)
    s5 = SR.conv_products(A, W, src, dst, koff, n_dst, R.FIVE) if g2 else None
    m = torch.tensor(float(6 * W.shape[1] + m_r + 8), dtype=torch.float64)
    gate(kernel, what, got, ref, bound, m, conv_mutants(A.double(), W.double(), src, dst, koff), bf16_got, fp32_got, s5)
    return ref


def wgrad_check_split(lib, what, got, A, ia, G, ig, koff, bf16_got, fp32_got=None, g2=True, kernel="pairs_wgrad_split", mutants=wgrad_mutants):
    """mutants: the regime tests' (a pair in the middle of the largest offset), or at full size SR.wgrad_mutants_resolved (see there)."""
    kvol, n = koff.shape[0] - 1, int(koff[-1])
    length = SR.split_tile_len(lib, n, A.shape[1], G.shape[1], kvol)
    ref, bound = SR.wgrad_gate(A, ia, G, ig, koff, length)
    s5 = SR.wgrad_products(A, ia, G, ig, koff, R.FIVE) if g2 else None
    tiles = (koff[1:] - koff[:-1] + length - 1) // length
    m = (6 * (length + tiles + 16) + 8).double().view(kvol, 1, 1)
    gate(kernel, what, got, ref, bound, m, mutants(A.double(), ia, G.double(), ig, koff), bf16_got, fp32_got, s5)
    return ref


# ---------------------------------------------------------------- every instantiation, synthetic pair lists
@pytest.mark.parametrize("w_t", [0, 1])
@pytest.mark.parametrize("ca,co,n_pairs,cols", GEMM_CASES)
def test_pair_gemm_split_every_column_block(env, ca, co, n_pairs, cols, w_t):
    """NT = 1, 2, 3, 4 with W stored (ca, co) and (co, ca); column tiles outside W; ca % 32 != 0 (ca = 4 included) takes the
    zero-filled reduction path."""
    spf, L = env
    g = gen(ca * 7 + co * 13 + n_pairs + w_t + 2)
    sizes = random_sizes(g, n_pairs, 27)
    n_src, n_dst = 5000, max(sizes) + 17
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    assert L.ftx_spconv_gemm_split_block_cols(co, n_pairs, 27) == cols
    A = randn(g, n_src, ca)
    Wl = randn(g, 27, ca, co, scale=(ca * 27) ** -0.5)
    Ws = Wl.transpose(1, 2).contiguous() if w_t else Wl
    Ad, Wd = A.cuda(), Ws.cuda()
    run = lambda **kw: spf._spconv_apply(Ad, Wd, d["src"], d["pos"], d["koff"], n_pairs, n_dst, co, w_t, **kw)   # noqa: E731
    out = run(operands="split")
    conv_check_split("pairs_gemm+reduce_split", f"{ca}->{co} wT={w_t}", out, A, Wl, src, dst, koff, n_dst, run(bf16=True), run())
    assert torch.equal(run(operands="split"), out)


@pytest.mark.parametrize("ca,cg,sides", WGRAD_CASES)
def test_wgrad_split_every_instantiation(env, ca, cg, sides):
    """Every reachable (MI, WMG) x (NI, WNG) pair of tile sides ((3,1) x (3,1) is sent to (2,2) x (3,1), as in fp32): the tiles of one
    wave split k-steps and products between four wave groups, the others k-steps between two or none."""
    spf, L = env
    assert S.wgrad_config(ca, cg) == (sides if sides != (3, 1, 3, 1) else (2, 2, 3, 1))
    g = gen(ca * 31 + cg + 2)
    sizes = random_sizes(g, 30000, 27)
    n_src, n_dst = 4000, max(sizes) + 5
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    A, G = randn(g, n_src, ca), randn(g, n_dst, cg)
    Ad, Gd = A.cuda(), G.cuda()
    run = lambda **kw: spf._spconv_wgrad(Ad, d["src"], Gd, d["dst"], d["koff"], int(koff[-1]), **kw)   # noqa: E731
    dW = run(operands="split")
    wgrad_check_split(L, f"{ca}x{cg} {sides}", dW, A, src, G, dst, koff, run(bf16=True), run())
    assert torch.equal(run(operands="split"), dW)


@pytest.mark.parametrize("kvol,ca,cg", [(27, 32, 32), (8, 128, 96), (5, 4, 64)])
def test_tile_edges_split(env, kvol, ca, cg):
    """Offset sizes around the 32-pair stages, the 128-pair GEMM tiles and this family's weight-gradient tile length L (L-1, L, L+1,
    many tiles), empty offsets; pair GEMM + reduce and weight gradient."""
    spf, L = env
    sizes, length = S.edge_sizes(L, ca, cg, kvol, tile_len=SR.split_tile_len)
    g = gen(kvol * 100 + ca + cg + 2)
    P = sum(sizes)
    assert SR.split_tile_len(L, P, ca, cg, kvol) == length
    n_src, n_dst = 3000, max(sizes) + 3
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    A, W, G = randn(g, n_src, ca), randn(g, kvol, ca, cg, scale=(ca * kvol) ** -0.5), randn(g, n_dst, cg)
    Ad, Wd, Gd = A.cuda(), W.cuda(), G.cuda()
    fwd = lambda **kw: spf._spconv_apply(Ad, Wd, d["src"], d["pos"], d["koff"], P, n_dst, cg, 0, **kw)   # noqa: E731
    out = fwd(operands="split")
    conv_check_split("pairs_gemm+reduce_split", f"edges kvol {kvol}", out, A, W, src, dst, koff, n_dst, fwd(bf16=True), fwd())
    assert torch.equal(fwd(operands="split"), out)
    wg = lambda **kw: spf._spconv_wgrad(Ad, d["src"], Gd, d["dst"], d["koff"], P, **kw)   # noqa: E731
    dW = wg(operands="split")
    ref = wgrad_check_split(L, f"edges kvol {kvol}", dW, A, src, G, dst, koff, wg(bf16=True), wg())
    assert torch.equal(wg(operands="split"), dW)
    empty = [k for k, c in enumerate(sizes) if c == 0]
    assert empty and bool((dW[empty] == 0).all()) and bool((ref[empty] == 0).all())


@pytest.mark.parametrize("e", S.DENSE, ids=[e["name"] for e in S.DENSE])
def test_dense_rows_split_with_and_without_bias(env, e):
    """functional.linear(operands="split") (bias) and rows_matmul(operands="split") (no bias) on 81 k rows: outputs, input gradients,
    dense-mode weight gradients."""
    spf, L = env
    n, ca, co = e["rows"], e["ca"], e["co"]
    g = gen(ca * 1000 + co + 2)
    x, W, b, go = randn(g, n, ca), randn(g, co, ca, scale=ca ** -0.5), randn(g, co), randn(g, n, co)
    assert L.ftx_spconv_gemm_split_block_cols(co, n, 0) == e["fwd"] and L.ftx_spconv_gemm_split_block_cols(ca, n, 0) == e["dgrad"]
    r, c, j = n // 2, ca // 2, co // 2
    x64, W64, g64, b64 = x.double(), W.double(), go.double(), b.double()
    idx, koff1 = torch.arange(n), torch.tensor([0, n])
    # the float64 references are the same with and without the bias: computed once, shared by both passes of the loop
    S_fwd, R_fwd, S5_fwd = x64 @ W64.T, x64.abs() @ W64.abs().T, R.gemm(x, W.T.contiguous(), R.FIVE)
    S_dx, R_dx, S5_dx = g64 @ W64, g64.abs() @ W64.abs(), R.gemm(go, W, R.FIVE)
    S_dw, R_dw, S5_dw = (g64.T @ x64)[None], (g64.abs().T @ x64.abs())[None], R.gemm(go.T.contiguous(), x, R.FIVE)[None]
    dw_mutants = SR.wgrad_mutants_resolved(g64, idx, x64, idx, koff1)

    def run(bias, **kw):
        xd, Wd = x.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
        if bias:
            y = spf.linear(xd, Wd, b.cuda().requires_grad_(True), **kw)
        else:
            y = spf.rows_matmul(xd, Wd.t().contiguous(), **kw)   # kernel (ca, co)
        y.backward(go.cuda())
        return y.detach(), xd.grad, Wd.grad

    for bias in (True, False):
        tag = e["name"] + (" linear" if bias else " matmul")
        (y, gx, gw), again, rounded, exact = run(bias, operands="split"), run(bias, operands="split"), run(bias, bf16=True), run(bias)
        for u, v in zip((y, gx, gw), again):
            assert torch.equal(u, v), tag
        add = b64 if bias else 0
        m = torch.tensor(float(6 * ca + int(bias) + 8), dtype=torch.float64)
        gate("rows_gemm_split", tag + " forward", y, S_fwd + add, m * U * (R_fwd + (b64.abs() if bias else 0)), m,
             [[((r,), -x64[r, c] * W64[:, c])], [((r,), x64[r, c] * (W64[:, c + 1] - W64[:, c]))]], rounded[0], exact[0], S5_fwd + add)
        m = torch.tensor(float(6 * co + 8), dtype=torch.float64)
        gate("rows_gemm_split", tag + " input gradient", gx, S_dx, m * U * R_dx, m,
             [[((r,), -g64[r, j] * W64[j])], [((r,), g64[r, j] * (W64[j + 1] - W64[j]))]], rounded[1], exact[1], S5_dx)
        # the dense-mode weight gradient: linear gives dW = go^T x, rows_matmul dK = x^T go (compared as go^T x: gw is (co, ca) either way)
        a_c, g_c = (co, ca) if bias else (ca, co)
        length = SR.split_tile_len(L, n, a_c, g_c, 1)
        m = torch.tensor(float(6 * (length + S.cdiv(n, length) + 16) + 8), dtype=torch.float64)
        gate("pairs_wgrad_split", tag + " weight gradient", gw[None], S_dw, m * U * R_dw, m, dw_mutants, rounded[2][None], exact[2][None], S5_dw)


def test_library_fallback_is_the_plain_fp32_gemm(env):
    """Shapes the tile kernel does not take (channels not a multiple of 4, above 512) go to the plain fp32 library GEMM in split mode:
    the bits of the default mode, not those of the bf16 fallback."""
    spf, _ = env
    g = gen(78)
    for ca, co in ((30, 18), (516, 32)):
        x, W, b = randn(g, 3000, ca).cuda(), randn(g, co, ca, scale=ca ** -0.5).cuda(), randn(g, co).cuda()
        assert torch.equal(spf.linear(x, W, b, operands="split"), spf.linear(x, W, b))
        assert torch.equal(spf.rows_matmul(x, W.t().contiguous(), operands="split"), spf.rows_matmul(x, W.t().contiguous()))
        assert not torch.equal(spf.linear(x, W, b, operands="split"), spf.linear(x, W, b, bf16=True))


def test_out_of_range_gather_gives_a_zero_row(env):
    """Source indices below 0 or past the last row give a zero pair row; every other row is the product of its gathered row."""
    spf, L = env
    g = gen(6)
    sizes = [300, 0, 517, 129]
    n_src, n_dst = 900, 600
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    bad = [3, 301, 700, 945]
    s = d["src"].clone()
    s[bad[0]], s[bad[1]], s[bad[2]], s[bad[3]] = -1, n_src, n_src + 1000, -7
    A, W = randn(g, n_src, 64), randn(g, 4, 64, 96, scale=0.1)
    Ad, Wd = A.cuda(), W.cuda()      # held until the launch has finished: the kernel reads them through raw pointers
    tmp = torch.full((sum(sizes), 96), float("nan"), device="cuda")
    spf.check(L.ftx_spconv_pairs_gemm_split(Ad.data_ptr(), n_src, s.data_ptr(), Wd.data_ptr(), 0, d["koff"].data_ptr(), sum(sizes), 64, 96,
                                            4, tmp.data_ptr(), spf._lib.stream()), "gemm")
    tmp = tmp.cpu()
    del Ad, Wd
    assert bool((tmp[bad] == 0).all())
    ok = torch.ones(sum(sizes), dtype=torch.bool)
    ok[bad] = False
    k_of = torch.repeat_interleave(torch.arange(4), torch.tensor(sizes))
    ref = torch.einsum("pc,pcd->pd", A.double()[src[ok]], W.double()[k_of[ok]])
    bound = (6 * 64 + 8) * U * torch.einsum("pc,pcd->pd", A.double().abs()[src[ok]], W.double().abs()[k_of[ok]])
    assert ratio(tmp[ok], ref, bound) <= 1.0


# ---------------------------------------------------------------- production layers at full size (G1)
@pytest.mark.parametrize("e", S.PRODUCTION, ids=[e["name"] for e in S.PRODUCTION])
def test_production_layer_split(env, bench_maps, e):
    spf, L = env
    km = get_map(bench_maps, e["map"])
    assert km.n_pairs == e["n_pairs"], (e["name"], km.n_pairs)
    kvol, ca, co, P = km.kvol, e["ca"], e["co"], km.n_pairs
    if e["form"] == "deconv":
        src_d, dst_d, n_src, n_dst, pos_f, pos_b = km.pair_out, km.pair_in, km.n_out, km.n_in, None, km.pos
    else:
        src_d, dst_d, n_src, n_dst, pos_f, pos_b = km.pair_in, km.pair_out, km.n_in, km.n_out, km.pos, (None if e["form"] == "down_dgrad" else km.pos_t)
    src, dst, koff = src_d.long().cpu(), dst_d.long().cpu(), km.koff.long().cpu()
    g = gen(len(e["name"]) + ca + co + 2)
    A, W, G = randn(g, n_src, ca), randn(g, kvol, ca, co, scale=(ca * kvol) ** -0.5), randn(g, n_dst, co)
    Ad, Wd, Gd = A.cuda(), W.cuda(), G.cuda()

    assert L.ftx_spconv_gemm_split_block_cols(co, P, kvol) == e["fwd"] and L.ftx_spconv_gemm_split_block_cols(ca, P, kvol) == e["dgrad"]
    if pos_f is None:
        fwd = lambda **kw: spf._spconv_direct(Ad, Wd, src_d, dst_d, km.koff, P, n_dst, co, 0, **kw)   # noqa: E731
        kernel = "pairs_gemm_scatter_split"
    else:
        fwd = lambda **kw: spf._spconv_apply(Ad, Wd, src_d, pos_f, km.koff, P, n_dst, co, 0, **kw)   # noqa: E731
        kernel = "pairs_gemm+reduce_split"
    out = fwd(operands="split")
    conv_check_split(kernel, e["name"] + " forward", out, A, W, src, dst, koff, n_dst, fwd(bf16=True), fwd(), g2=False)
    assert torch.equal(fwd(operands="split"), out)
    Wt = W.transpose(1, 2)
    if pos_b is None:
        bwd = lambda **kw: spf._spconv_direct(Gd, Wd, dst_d, src_d, km.koff, P, n_src, ca, 1, **kw)   # noqa: E731
        kernel = "pairs_gemm_scatter_split"
    else:
        bwd = lambda **kw: spf._spconv_apply(Gd, Wd, dst_d, pos_b, km.koff, P, n_src, ca, 1, **kw)   # noqa: E731
        kernel = "pairs_gemm+reduce_split"
    gin = bwd(operands="split")
    conv_check_split(kernel, e["name"] + " data gradient", gin, G, Wt, dst, src, koff, n_src, bwd(bf16=True), bwd(), g2=False)
    assert torch.equal(bwd(operands="split"), gin)
    wg = lambda **kw: spf._spconv_wgrad(Ad, src_d, Gd, dst_d, km.koff, P, **kw)   # noqa: E731
    dW = wg(operands="split")
    wgrad_check_split(L, e["name"] + " weight gradient", dW, A, src, G, dst, koff, wg(bf16=True), wg(), mutants=SR.wgrad_mutants_resolved)
    assert torch.equal(wg(operands="split"), dW)


def test_conv_bn_node_matches_sparse_conv_then_batch_norm(env, bench_maps):
    """The fused node (operands="split") against sparse_conv(operands="split") + batch_norm on the 192 -> 128 layer of level 4: the
    convolution output it keeps, its output and the gradients of input, weight, gamma and beta, bit for bit; its own repeatability;
    and the launch kinds say which family ran."""
    spf, L = env
    km = bench_maps.kernel_map(3, 4, 1)
    ca, co, kvol, n = 192, 128, 27, km.n_out
    g = gen(1921)
    A, W = randn(g, n, ca), randn(g, kvol, ca, co, scale=(ca * kvol) ** -0.5)
    gam, bet, gy = torch.rand(co, generator=g).float() + 0.5, randn(g, co), randn(g, n, co).cuda()

    def fused():
        Ad, Wd = A.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
        gd, bd = gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
        y = spf.conv_bn_train(Ad, Wd, km, False, gd, bd, torch.zeros(co, device="cuda"), torch.ones(co, device="cuda"), 0.1, 1e-5, relu=True,
                              operands="split")
        x = y.grad_fn.saved_tensors[2].detach().clone()
        y.backward(gy)
        return x, y.detach(), Ad.grad, Wd.grad, gd.grad, bd.grad

    Ad, Wd = A.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
    gd, bd = gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
    x2 = spf.sparse_conv(Ad, Wd, km, False, operands="split")
    y2 = spf.batch_norm(x2, gd, bd, torch.zeros(co, device="cuda"), torch.ones(co, device="cuda"), True, 0.1, 1e-5, relu=True)
    y2.backward(gy)
    spf.LAUNCH_LOG = []
    try:
        a = fused()
        torch.cuda.synchronize()
        kinds = {k for k, *_ in spf.LAUNCH_LOG if k.startswith("spconv_")}
    finally:
        spf.LAUNCH_LOG = None
    assert kinds == {"spconv_pairs_gemm_split", "spconv_pairs_wgrad_split", "spconv_reduce"}, kinds
    b = fused()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[0], x2.detach())
    for name, u, v in zip(("y", "gA", "gW", "ggamma", "gbeta"), a[1:], (y2.detach(), Ad.grad, Wd.grad, gd.grad, bd.grad)):
        assert torch.equal(u, v), name
    assert not torch.equal(a[0], spf.sparse_conv(A.cuda(), W.cuda(), km, False).detach()), "the split mode returned the fp32 family's bits"


# ---------------------------------------------------------------- model level
def _model(seed, **switches):
    from fusiontransformer_amd.models.build import build_model
    from oracle import ft_oracle as O
    cfg = small_cfg("middle")
    torch.manual_seed(seed)
    oracle = O.build_model(dict(cfg.MODEL))
    for k, v in switches.items():
        cfg.MODEL[k] = v
    model, _, _ = build_model(cfg)
    model.load_state_dict(oracle.state_dict())
    return cfg, oracle, model.cuda()


def test_lidar_split_eval_logits_meet_the_fp32_gate():
    """Middle fusion, small frames, eval: lidar_split=True against the PLAIN CPU oracle within 1e-3 max-abs, the fp32 path's gate
    (tests/test_model_gpu.py), image logits unchanged.  The rms distance to the oracle is at most twice that of the default path (two
    fp32-class summation orders sit at the same distance from the oracle, not at an equal one) and at most a tenth of lidar_bf16's
    (the factor the bf16 test demands between its two oracles).
    Measured on an MI355X: max |split - oracle| 8.9e-8; rms_split 1.32e-8, rms_f32 1.37e-8, rms_bf16 7.32e-5 (split / f32 0.96, bf16 /
    split 5 500); image logits 9.7e-7 from the oracle and bit-identical to the default path's."""
    from fusiontransformer_amd.data.synth import make_batch
    batch = make_batch([0, 1], max_points=2500)
    keys = ("lidar_seg_logit", "lidar_seg_logit2")
    outs = {}
    for name, sw in (("f32", {}), ("bf16", dict(lidar_bf16=True)), ("split", dict(lidar_split=True))):
        cfg, oracle, model = _model(3, **sw)
        oracle.eval(); model.eval()
        with torch.no_grad():
            outs[name] = {k: v.cpu() for k, v in model(product_inputs(batch)).items()}
            if name == "f32":
                plain = oracle(oracle_inputs(batch))
        del model
    rms = lambda a: max(float((a[k] - plain[k]).double().pow(2).mean().sqrt()) for k in keys)   # noqa: E731
    rms_f32, rms_bf16, rms_split = rms(outs["f32"]), rms(outs["bf16"]), rms(outs["split"])
    err = max((outs["split"][k] - plain[k]).abs().max().item() for k in keys)
    err_img = max((outs["split"][k] - plain[k]).abs().max().item() for k in ("img_seg_logit", "img_seg_logit2"))
    print(f"\nlidar_split logits vs the plain oracle: max {err:.3g}, rms_split {rms_split:.3g}, rms_f32 {rms_f32:.3g}, rms_bf16 {rms_bf16:.3g}; "
          f"image logits vs oracle {err_img:.3g}")
    assert err <= 1e-3, err
    assert err_img <= 1e-3, err_img
    for k in ("img_seg_logit", "img_seg_logit2"):
        assert torch.equal(outs["split"][k], outs["f32"][k]), k
    assert rms_split <= 2 * rms_f32, (rms_split, rms_f32)
    assert rms_split <= rms_bf16 / 10, (rms_split, rms_bf16)


def test_lidar_split_train_step_matches_oracle():
    """One training step with lidar_split at the gates of tests/test_model_gpu.py test_train_step_matches_oracle, unchanged: logits
    within 1e-3, losses within 1e-4, every gradient within 5e-2 L2-relative of the float64 oracle, running statistics within 1e-4."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.trainer import fusion_losses
    from oracle import ft_oracle as O
    cfg, oracle, model = _model(1, lidar_split=True)
    assert model.lidar_backbone.lidar_split
    oracle64 = O.build_model(dict(small_cfg("middle").MODEL)).double()
    oracle64.load_state_dict(oracle.state_dict())
    oracle64.train()
    batch = make_batch([2, 3], max_points=2000)
    oracle.train(); model.train()
    with torch.no_grad():
        oracle.eval(); oracle(oracle_inputs(batch)); oracle.train()
    li = oracle.lidar_backbone.last_index
    g = torch.Generator().manual_seed(5)
    masks = {"y1": (torch.rand(li["x4"].C.shape[0], 256, generator=g) > 0.3).float(),
             "y3": (torch.rand(li["x2"].C.shape[0], 128, generator=g) > 0.3).float()}
    oracle.lidar_backbone.dropout_masks = masks
    model.lidar_backbone.dropout_masks = {k: v.cuda() for k, v in masks.items()}
    cw = torch.tensor(cfg.TRAIN.CLASS_WEIGHTS)
    ref = oracle(oracle_inputs(batch))
    l2r, l3r = O.fusion_losses(ref, torch.from_numpy(batch["seg_label"]), cw, 0.1, True)
    (l2r + l3r).backward()
    pin = product_inputs(batch)
    out = model(pin)
    l2, l3 = fusion_losses(out, pin["seg_label"], cw.cuda(), 0.1, True)
    (l2 + l3).backward()
    for k in ref:
        err = (out[k].detach().cpu() - ref[k].detach()).abs().max().item()
        assert err <= 1e-3, (k, err)
    assert abs(l2.item() - l2r.item()) < 1e-4 and abs(l3.item() - l3r.item()) < 1e-4
    oracle64.lidar_backbone.dropout_masks = {k: v.double() for k, v in masks.items()}
    i64 = oracle_inputs(batch)
    i64["img"], i64["lidar"].F = i64["img"].double(), i64["lidar"].F.double()
    a64, b64 = O.fusion_losses(oracle64(i64), torch.from_numpy(batch["seg_label"]), cw.double(), 0.1, True)
    (a64 + b64).backward()
    p64, pp = dict(oracle64.named_parameters()), dict(model.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in p64.values() if p.grad is not None)
    report = []
    for name, p in p64.items():
        if p.grad is None:
            assert pp[name].grad is None or pp[name].grad.abs().max().item() == 0, name
            continue
        gp = pp[name].grad.cpu().double()
        floor = 1e-4 * gmax * p.numel() ** 0.5
        report.append(((gp - p.grad).norm().item() / max(p.grad.norm().item(), floor), p.grad.norm().item(), name))
    report.sort(reverse=True)
    print(f"\nlidar_split train step: worst gradient rel-L2 {report[0][0]:.3g} ({report[0][2]})")
    assert report[0][0] < 5e-2, report[:5]
    bo, bp = dict(oracle.named_buffers()), dict(model.named_buffers())
    for name, b in bo.items():
        if b.dtype.is_floating_point:
            assert (bp[name].cpu() - b).abs().max().item() < 1e-4, name
        else:
            assert int(bp[name].item()) == int(b.item()), name


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
    kinds = _step_log(_model(4)[2], pin)
    assert "spconv_pairs_gemm" in kinds and "spconv_ostat" in kinds and not any(k.endswith("_split") for k in kinds), sorted(set(kinds))
    kinds = _step_log(_model(4, lidar_split=True)[2], pin)
    sp = {k for k in kinds if k.startswith("spconv_")}
    assert sp <= {"spconv_pairs_gemm_split", "spconv_pairs_wgrad_split", "spconv_reduce", "spconv_ostat"}, sp
    assert {"spconv_pairs_gemm_split", "spconv_pairs_wgrad_split"} <= sp, sp
    assert "spconv_ostat" in sp, "a split layer keeps the output-stationary route where the fp32 path takes it"


def test_lidar_split_graphed_two_stream_step_is_bit_identical_to_eager_twin():
    """With lidar_split=True, a training step with the graphed trunk on two streams against an eager-trunk, one-stream twin: logits
    and every gradient bit for bit (capturing step and a replay)."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.trainer import fusion_losses
    pin = product_inputs(make_batch([2, 3], max_points=3000))

    def run(graphs, steps):
        cfg, oracle, model = _model(5, lidar_split=True)
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


@pytest.mark.parametrize("native_index", [False, True], ids=["index per op", "native index"])
def test_native_eval_executor_with_lidar_split_is_bit_identical(native_index):
    """The eval executor on against off with lidar_split, and the same with the native index build on: every layer record carries
    mode 2 and the logits are the same bits; they are not the default mode's bits."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.native_eval import NativeEval
    from tests.test_native_train_gpu import _pair
    from tests.test_native_eval_gpu import same
    batch = make_batch([2], max_points=1700)
    for kind in ("lidar", "middle"):
        _, model, _, net, _ = _pair(kind, seed=6)
        model.eval()
        net.set_split(True)
        net.set_native_index(native_index)
        with torch.no_grad():
            off = model(product_inputs(batch))
            net.set_native_eval(True)
            on = model(product_inputs(batch))
        torch.cuda.synchronize()
        assert isinstance(net._native, NativeEval) and net._native.arenas and all(int(r["bf16"]) == 2 for r in net._native.layers)
        for k in off:
            assert same(on[k], off[k]), (kind, k)
        net.set_split(False)
        with torch.no_grad():
            fp32 = model(product_inputs(batch))
        assert not torch.equal(fp32["lidar_seg_logit"], on["lidar_seg_logit"]), "the split switch changed nothing"


def test_native_training_executor_with_lidar_split_is_bit_identical():
    """The training executor on against a twin with it off, both with lidar_split: logits, losses, every gradient, every parameter
    after Adam and every BatchNorm buffer bit for bit, over two steps on batches of different size."""
    from fusiontransformer_amd.data.synth import make_batch
    from tests.test_native_train_gpu import _assert_executor_ran, _pair, _twin_steps
    a, b = make_batch([0, 1], max_points=2500), make_batch([2], max_points=1700)
    cfg, model, twin, net, net_twin = _pair("middle", seed=5)
    for n in (net, net_twin):
        n.set_split(True)
    net.set_native_train(True)
    preds = _twin_steps("middle", cfg, model, twin, net, net_twin, [(b, None), (a, None)])
    _assert_executor_ran(net, preds, 2)
    assert all(int(r["bf16"]) == 2 for r in net._native_tr.layers)
