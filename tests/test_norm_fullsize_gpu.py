"""BatchNorm (csrc/ftx_bn.hip), add + LayerNorm (csrc/ftx_layernorm.hip) and the fused sample-down (csrc/ftx_sampledown.hip) at
production size, against the float64 restatements of tests/norm_ref.py.

Sizes come from make_batch([0, 1, 2, 3]): the voxel levels and kernel maps of bench.py's first batch, its 81 237 point rows, the
578-token ViT trunk at batch 1, 2 and 4 (the three rows-per-block regimes of the LayerNorm backward), and the 370 x 1226 / 900 x 1600
images.  Every gate is |got - ref| <= bound with the bound derived, in norm_ref, from the rounding steps the kernel takes, and is
stage-wise: statistics, then the apply, then the backward, each evaluated in float64 on the kernel's own float32 output of the stage
before.  Each gate must also reject two planted mutants of its reference.  Exact claims (the residual gradient dy * mask, the sample-
down sums on dyadic data, the two ReLU-mask modes of the BatchNorm backward) use torch.equal / assert_array_equal.

The ReLU mask of the backward is taken from the kernel's own y > 0: a float64 pre-activation within rounding of 0 must not flip the
reference."""
import numpy as np
import pytest
import torch

from tests import norm_ref as R
from tests import spconv_regimes as S
from tests.norm_ref import U, conv_check, conv_mutants, conv_ref, f32, gen, randn, wgrad_check, whole
from tests.test_spconv_regimes_gpu import bench_maps, get_map  # noqa: F401

pytestmark = pytest.mark.gpu

KERNELS = set()      # the kernels this module gates (R.WORST is shared with the sparse-convolution modules)
BRANCH = {}          # conv_bn_train case -> launches it made
NOTES = []
MOM = float(np.float32(0.1))
EPS = float(np.float32(1e-5))
EPS_LN = float(np.float32(1e-6))
POINT_ROWS = S.DENSE_ROWS


@pytest.fixture(scope="module")
def env():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield spf, _lib.load()
    print("\nnormalisation: worst error / bound per kernel: " + ", ".join(f"{k} {R.WORST[k]:.3g}" for k in sorted(KERNELS)))
    print("conv_bn_train branches: " + "; ".join(f"{k}: {v}" for k, v in BRANCH.items()))
    print("\n".join(NOTES))


def gate(kernel, what, got, ref, bound, mutants):
    KERNELS.add(kernel)
    R.check(kernel, what, got, ref, bound, mutants)


def host(t):
    return t.detach().cpu().double()


def launches(spf):
    out = [(k, m.get("reads")) for k, _, _, m in spf.LAUNCH_LOG]
    spf.LAUNCH_LOG.clear()
    return out


# ---------------------------------------------------------------- BatchNorm stages
def gate_bn_stats(kernel, what, x, mean_k, invstd_k, rm, rv, rm0, rv0):
    """Batch statistics against float64 of the kernel's own input x; running statistics from the kernel's float32 mean."""
    n = x.shape[0]
    mu, var = R.bn_stats(x)
    invstd = R.bn_invstd(var, EPS)
    mb, ib = R.bn_stats_bounds(x, mu, invstd)
    r = int(torch.argmax((x - mu).abs().sum(1)))
    mu_d, var_d = R.bn_stats(x, drop_row=r)
    gate(kernel, what + " batch mean", mean_k, mu, mb, [whole(mu_d - mu), whole((x[r] - mu) / n)])
    gate(kernel, what + " batch invstd", invstd_k, invstd, ib,
         [whole(R.bn_invstd(var_d, EPS) - invstd), whole(R.bn_invstd(var * n / (n - 1), EPS) - invstd)])
    mk = host(mean_k)
    rm_ref, rv_ref = R.bn_running(rm0, rv0, mk, var, n, MOM)
    rmb, rvb = R.bn_running_bounds(rm0, rv0, mk, var, x, MOM)
    gate(kernel, what + " running mean", rm, rm_ref, rmb, [whole(MOM * (mu_d - mu)), whole(R.bn_running(rm0, rv0, mk, var, n, 1 - MOM)[0] - rm_ref)])
    gate(kernel, what + " running var", rv, rv_ref, rvb,
         [whole(R.bn_running(rm0, rv0, mk, var, n, MOM, unbiased=False)[1] - rv_ref), whole(R.bn_running(rm0, rv0, mk, var_d, n, MOM)[1] - rv_ref)])
    return mk, host(invstd_k)


def gate_bn_apply(kernel, what, y, x, mk, ik, gamma, beta, res, relu):
    ref, pre, bound = R.bn_apply(x, mk, ik, gamma, beta, res, relu)
    r = int(torch.argmax(pre.abs().sum(1)))
    if relu:        # one element's mask flipped: the most negative pre-activation passed through
        k = int(torch.argmin(pre.reshape(-1)))
        ix = (k // pre.shape[1], k % pre.shape[1])
        first = [(ix, pre[ix])]
    else:           # row r's xhat term dropped
        first = [((r,), -(x[r] - mk) * ik * gamma)]
    gate(kernel, what + " output", y, ref, bound, [first, [((r,), ref[r - 1] - ref[r])]])


def gate_bn_backward(kernel, what, gy, x, mk, ik, gamma, mask, gbeta, ggamma, gres, gx=None):
    """d beta, d gamma, the residual gradient (exact) and, when given, the input gradient; returns (reference gx, its bound)."""
    out, b = R.bn_backward(gy, x, mk, ik, gamma, mask)
    r = int(torch.argmax((out["dy"] * (x - mk)).abs().sum(1)))
    drop, _ = R.bn_backward(gy, x, mk, ik, gamma, mask, drop_row=r)
    if mask is not None:
        flip = mask.clone()
        k = int(torch.argmax((gy * (x - mk) * mask).abs().reshape(-1)))
        flip.view(-1)[k] = ~flip.view(-1)[k]
    else:
        flip = torch.ones_like(x, dtype=torch.bool)
        flip.view(-1)[int(torch.argmax((gy * (x - mk)).abs().reshape(-1)))] = False
    alt, _ = R.bn_backward(gy, x, mk, ik, gamma, flip)
    for key, got in (("dbeta", gbeta), ("dgamma", ggamma)):
        gate(kernel + " backward", f"{what} {key}", got, out[key], b[key], [whole(drop[key] - out[key]), whole(alt[key] - out[key])])
    if gx is not None:
        gate(kernel + " backward", what + " gx", gx, out["gx"], b["gx"], [whole(drop["gx"] - out["gx"]), whole(alt["gx"] - out["gx"])])
    if gres is not None:
        assert torch.equal(gres.cpu(), out["dy"].float()), what + ": residual gradient != gy * mask"
        assert not torch.equal(gres.cpu(), gy.float()) and not torch.equal(gres.cpu(), alt["dy"].float())
    return out["gx"], b["gx"]


# ---------------------------------------------------------------- conv_bn_train on production layers
CONV_BN = [
    dict(name="a stem 4->32 L1 relu", map=("subm", 1), transposed=False, ca=4, co=32, res=False,
         fwd=["spconv_ostat", "bn_fwd"], bn_reads=1, bwd_reads=4),
    dict(name="b 32->32 L2 res+relu", map=("subm", 2), transposed=False, ca=32, co=32, res=True,
         fwd=["spconv_ostat", "bn_fwd"], bn_reads=2, bwd_reads=6),
    dict(name="c 96->96 L1 res+relu", map=("subm", 1), transposed=False, ca=96, co=96, res=True,
         fwd=["spconv_pairs_gemm", "spconv_reduce", "bn_fwd"], bn_reads=2, bwd_reads=6),
    dict(name="d deconv 96->96 L2->L1 relu", map=("down", 1), transposed=True, ca=96, co=96, res=False,
         fwd=["spconv_pairs_gemm", "bn_fwd"], bn_reads=2, bwd_reads=4),
]


@pytest.mark.parametrize("e", CONV_BN, ids=[e["name"] for e in CONV_BN])
def test_conv_bn_train_at_full_size(env, bench_maps, monkeypatch, e):  # noqa: F811
    """conv_bn_train with ReLU: the convolution output it keeps, batch and running statistics, y, d beta / d gamma, the residual
    gradient (exact), the input gradient and the weight gradient.  Branches: a, b output-stationary conv + statistics, then
    ftx_bn_train_fwd_totals; c pair GEMM + ftx_spconv_reduce_stats (c = 96: RL = 10 leaves 16 threads of a block idle); d the direct
    (scatter) transposed conv, then ftx_bn_train_fwd with its own statistics pass.  Without a residual the backward recomputes the
    ReLU mask from x (bn_bwd reads 4 row matrices), with one it reads y (6)."""
    spf, L = env
    km = get_map(bench_maps, e["map"])
    tr, ca, co, kvol = e["transposed"], e["ca"], e["co"], km.kvol
    if tr:
        src_d, dst_d, n_src, n = km.pair_out, km.pair_in, km.n_out, km.n_in
        assert km.fine_bijective
    else:
        src_d, dst_d, n_src, n = km.pair_in, km.pair_out, km.n_in, km.n_out
    src, dst, koff = src_d.long().cpu(), dst_d.long().cpu(), km.koff.long().cpu()
    g = gen(ca * 100 + co + len(e["name"]))
    A, W = randn(g, n_src, ca), randn(g, kvol, ca, co, scale=(ca * kvol) ** -0.5)
    gam, bet, gy = torch.rand(co, generator=g).float() + 0.5, randn(g, co, scale=0.5), randn(g, n, co)
    res = randn(g, n, co) if e["res"] else None
    rm0, rv0 = randn(g, co, scale=0.1), torch.rand(co, generator=g).float() + 0.5
    Ad, Wd = A.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
    gd, bd = gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
    resd = res.cuda().requires_grad_(True) if res is not None else None
    rm, rv = rm0.cuda(), rv0.cuda()
    monkeypatch.setattr(spf, "LAUNCH_LOG", [])
    y = spf.conv_bn_train(Ad, Wd, km, tr, gd, bd, rm, rv, MOM, EPS, residual=resd, relu=True)
    fwd = launches(spf)
    _, _, x_gpu, _, _, _, stats = y.grad_fn.saved_tensors
    y.backward(gy.cuda())
    bwd = launches(spf)
    torch.cuda.synchronize()
    BRANCH[e["name"]] = " ".join(k for k, _ in fwd) + " | " + " ".join(k for k, _ in bwd)
    assert [k for k, _ in fwd] == e["fwd"] and fwd[-1][1] == e["bn_reads"], fwd
    assert bwd[0] == ("bn_bwd", e["bwd_reads"]), bwd

    KERNELS.add("conv_bn conv")
    conv_check("conv_bn conv", e["name"] + " conv output", x_gpu, A, W, src, dst, koff, n)
    x = host(x_gpu)
    mk, ik = gate_bn_stats("bn statistics", e["name"], x, stats[0], stats[1], rm, rv, rm0.double(), rv0.double())
    g64, b64, r64 = gam.double(), bet.double(), (res.double() if res is not None else None)
    gate_bn_apply("bn apply", e["name"], y, x, mk, ik, g64, b64, r64, True)
    mask = y.detach().cpu() > 0
    gx, E_gx = gate_bn_backward("bn", e["name"], gy.double(), x, mk, ik, g64, mask, bd.grad, gd.grad, resd.grad if res is not None else None)
    Wt = W.double().transpose(1, 2)
    ref = conv_ref(gx, Wt, dst, src, koff, n_src)
    bound = (co + kvol + 8) * U * conv_ref(gx.abs(), Wt.abs(), dst, src, koff, n_src) + conv_ref(E_gx, Wt.abs(), dst, src, koff, n_src)
    gate("conv_bn input gradient", e["name"] + " input gradient", Ad.grad, ref, bound, conv_mutants(gx, Wt, dst, src, koff))
    KERNELS.add("pairs_wgrad(conv_bn)")
    wgrad_check(L, "pairs_wgrad(conv_bn)", e["name"] + " weight gradient", Wd.grad, A, src, gx, dst, koff, extra=E_gx)


# ---------------------------------------------------------------- standalone batch_norm
BN_CASES = [  # (name, rows, channels, residual, relu)
    ("point rows x 256 relu", POINT_ROWS, 256, False, True),
    ("point rows x 128 relu", POINT_ROWS, 128, False, True),
    ("point rows x 96 relu", POINT_ROWS, 96, False, True),
    ("1x1 down L4 x 64", S.BENCH_VOXELS[4], 64, False, False),
    ("1x1 down L16 x 256", S.BENCH_VOXELS[16], 256, False, False),
    ("1x1 down L1 x 96", S.BENCH_VOXELS[1], 96, False, False),
    ("tokens 2304 x 96", 2304, 96, False, False),
    ("unfused L1 x 96 res+relu", S.BENCH_VOXELS[1], 96, True, True),
]


@pytest.mark.parametrize("name,n,c,res,relu", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_batch_norm_train_at_full_size(env, monkeypatch, name, n, c, res, relu):
    """functional.batch_norm (training): statistics pass + apply, then the backward (ReLU mask recomputed from x without a residual,
    read from y with one): every stage gated, the residual gradient exact."""
    spf, _ = env
    g = gen(n + c)
    x = randn(g, n, c) * 1.3 + randn(g, c)
    gam, bet, gy = torch.rand(c, generator=g).float() + 0.5, randn(g, c, scale=0.5), randn(g, n, c)
    r = randn(g, n, c) if res else None
    rm0, rv0 = randn(g, c, scale=0.1), torch.rand(c, generator=g).float() + 0.5
    xd, gd, bd = x.cuda().requires_grad_(True), gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
    rd = r.cuda().requires_grad_(True) if res else None
    rm, rv = rm0.cuda(), rv0.cuda()
    monkeypatch.setattr(spf, "LAUNCH_LOG", [])
    y = spf.batch_norm(xd, gd, bd, rm, rv, True, MOM, EPS, residual=rd, relu=relu)
    _, _, _, _, mean_k, invstd_k = y.grad_fn.saved_tensors
    y.backward(gy.cuda())
    assert launches(spf) == [("bn_fwd", 2 + res), ("bn_bwd", 2 * (2 + (relu and res)))]
    x64 = x.double()
    mk, ik = gate_bn_stats("bn statistics", name, x64, mean_k, invstd_k, rm, rv, rm0.double(), rv0.double())
    r64 = r.double() if res else None
    gate_bn_apply("bn apply", name, y, x64, mk, ik, gam.double(), bet.double(), r64, relu)
    mask = (y.detach().cpu() > 0) if relu else None
    gate_bn_backward("bn", name, gy.double(), x64, mk, ik, gam.double(), mask, bd.grad, gd.grad, rd.grad if res else None, xd.grad)


@pytest.mark.parametrize("n,c,res", [(S.BENCH_VOXELS[1], 96, True), (POINT_ROWS, 256, False)])
def test_batch_norm_eval_at_full_size(env, n, c, res):
    """bn_apply_eval_kernel with ReLU (and a residual): running statistics, not the batch's; the running statistics stay as they were."""
    spf, _ = env
    g = gen(7 * n + c)
    x = randn(g, n, c) * 1.3 + randn(g, c)
    gam, bet = torch.rand(c, generator=g).float() + 0.5, randn(g, c, scale=0.5)
    r = randn(g, n, c) if res else None
    rm0, rv0 = randn(g, c, scale=0.3), torch.rand(c, generator=g).float() + 0.5
    rm, rv = rm0.cuda(), rv0.cuda()
    y = spf.batch_norm(x.cuda(), gam.cuda(), bet.cuda(), rm, rv, False, MOM, EPS, residual=r.cuda() if res else None, relu=True)
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    x64, r64 = x.double(), (r.double() if res else None)
    ref, pre, bound = R.bn_eval(x64, rm0.double(), rv0.double(), EPS, gam.double(), bet.double(), r64, True)
    mu, var = R.bn_stats(x64)
    batch, _, _ = R.bn_apply(x64, mu, R.bn_invstd(var, EPS), gam.double(), bet.double(), r64, True)
    k = int(torch.argmin(pre.reshape(-1)))
    ix = (k // c, k % c)
    gate("bn eval", f"eval {n}x{c}", y, ref, bound, [whole(batch - ref), [(ix, pre[ix])]])


def test_batch_norm_remask_matches_the_stored_mask(env):
    """The backward's recomputed ReLU mask (the default without a residual) against the mask read from y (remask=False) where
    pre-activations are the exact residual of a product, of either sign, or exactly 0.

    Planted columns take four distinct x values; after one forward, beta_j = -f32(t gamma_j) with t = f32(f32(x0 - mean_j) invstd_j)
    for the shared value x0, so bn_affine(x0) = fma(t, gamma_j, beta_j) is the rounding residual of t gamma_j (0 when gamma_j = 1).
    Beta does not move the statistics, so a second forward keeps them bit for bit, and the two backwards must agree bit for bit."""
    spf, _ = env
    n, c, planted = POINT_ROWS, 256, 32
    g = gen(256)
    x = randn(g, n, c)
    levels = torch.tensor([-1.0, -0.25, 0.5, 1.25])
    x[:, :planted] = levels[torch.randint(0, 4, (n, planted), generator=g)]
    gam = torch.rand(c, generator=g).float() + 0.5
    gam[:planted // 2] = 1.0
    bet, gy = randn(g, c, scale=0.5), randn(g, n, c)
    xd, gd = x.cuda().requires_grad_(True), gam.cuda().requires_grad_(True)
    y0 = spf.batch_norm(xd, gd, bet.cuda(), None, None, True, MOM, EPS, relu=True)
    mean0, inv0 = (t.clone() for t in y0.grad_fn.saved_tensors[4:6])
    mk, ik = mean0.cpu(), inv0.cpu()
    t = ((torch.tensor(0.5) - mk[:planted]) * ik[:planted])             # float32: two roundings, as bn_affine
    bet[:planted] = -(t * gam[:planted])
    bd = bet.cuda().requires_grad_(True)

    def run(remask=True):
        xd.grad = gd.grad = bd.grad = None
        y = spf.batch_norm(xd, gd, bd, None, None, True, MOM, EPS, relu=True, remask=remask)
        stats = [t.clone() for t in y.grad_fn.saved_tensors[4:6]]
        y.backward(gy.cuda())
        return y, stats, xd.grad.clone(), gd.grad.clone(), bd.grad.clone()

    y, stats, gx_a, gg_a, gb_a = run()
    assert torch.equal(stats[0], mean0) and torch.equal(stats[1], inv0)
    y_b, _, gx_b, gg_b, gb_b = run(remask=False)
    assert torch.equal(y, y_b)
    assert torch.equal(gx_a, gx_b) and torch.equal(gg_a, gg_b) and torch.equal(gb_a, gb_b)
    yc = y.detach().cpu()
    at = x[:, :planted] == 0.5
    zeros, tiny = int(((yc[:, :planted] == 0) & at).sum()), int(((yc[:, :planted] > 0) & (yc[:, :planted] < 1e-6) & at).sum())
    assert int(((yc[:, :planted // 2] == 0) & at[:, :planted // 2]).sum()) == int(at[:, :planted // 2].sum())   # gamma 1: exactly 0
    assert zeros > 1000 and tiny > 1000, (zeros, tiny)
    x64 = x.double()
    mask = yc > 0
    gate_bn_apply("bn apply", "remask", y, x64, mk.double(), ik.double(), gam.double(), bet.double(), None, True)
    for gx, gg, gb in ((gx_a, gg_a, gb_a), (gx_b, gg_b, gb_b)):
        gate_bn_backward("bn", "remask", gy.double(), x64, mk.double(), ik.double(), gam.double(), mask, gb, gg, None, gx)


# ---------------------------------------------------------------- add + LayerNorm
def ln_gates(what, s, stats, w, b, h, gh, gs, gx, gparams, vpl, k, y_bias_grad=None):
    mean_k, rstd_k = host(stats[0]), host(stats[1])
    mean, _ = R.ln_stats(s, EPS_LN)
    _, rstd = R.ln_stats(s, EPS_LN, mean_k)
    mb, rb = R.ln_stats_bounds(s, rstd, vpl)
    j = int(torch.argmax(s.abs().sum(0)))
    gate("layernorm statistics", what + " mean", stats[0], mean, mb,
         [whole(R.ln_stats(s, EPS_LN, drop_col=j)[0] - mean), whole(mean * 768 / 767 - mean)])
    gate("layernorm statistics", what + " rstd", stats[1], rstd, rb,
         [whole(R.ln_stats(s, EPS_LN, mean_k, ddof=1)[1] - rstd), whole(R.ln_stats(s, EPS_LN, mean_k, drop_col=j)[1] - rstd)])
    href, hb = R.ln_apply(s, mean_k, rstd_k, w, b)
    md = R.ln_stats(s, EPS_LN, drop_col=j)[0]
    rd = R.ln_stats(s, EPS_LN, mean_k, ddof=1)[1]
    gate("layernorm apply", what + " h", h, href, hb, [whole(R.ln_apply(s, md, rstd_k, w, b)[0] - href), whole(R.ln_apply(s, mean_k, rd, w, b)[0] - href)])
    out, bb = R.ln_backward(gh, gs, s, w, mean_k, rstd_k, vpl, k)
    alt, _ = R.ln_backward(gh, gs, s, w, md, rstd_k, vpl, k)
    if gs is not None:
        first = whole(R.ln_backward(gh, gs, s, w, mean_k, rstd_k, vpl, k, add_gs=False)[0]["gx"] - out["gx"])
    else:
        first = whole(R.ln_backward(gh, gs, s, w, mean_k, rd, vpl, k)[0]["gx"] - out["gx"])
    gate("layernorm backward", what + " gx", gx, out["gx"], bb["gx"], [first, whole(alt["gx"] - out["gx"])])
    xh = (s - mean_k[:, None]) * rstd_k[:, None]
    r = int(torch.argmax((gh * xh).abs().sum(1)))
    gate("layernorm backward", what + " d gamma", gparams[0], out["dgamma"], bb["dgamma"],
         [whole(-gh[r] * xh[r]), whole((gh[r - 1] - gh[r]) * xh[r])])
    gate("layernorm backward", what + " d beta", gparams[1], out["dbeta"], bb["dbeta"], [whole(-gh[r]), whole(gh[r - 1] - gh[r])])
    if y_bias_grad is not None:
        g64 = host(gx)
        ref, cb = R.ln_colsum(g64, k)
        gate("layernorm backward", what + " d y_bias", y_bias_grad, ref, cb, [whole(-g64[r]), whole(-gs.sum(0))])


@pytest.mark.parametrize("rows", [578, 1156, 2312])
def test_add_layer_norm_at_full_size(env, rows):
    """s = x + (y + y_bias), LayerNorm(s), C = 768 (VPL = 3), at batch 1, 2 and 4 of the trunk: 4, 8 and 16 rows per backward block
    (1, 2 and 4 rows per wave)."""
    spf, _ = env
    C = 768
    g = gen(rows)
    x, y, yb = randn(g, rows, C), randn(g, rows, C), randn(g, C, scale=0.1)
    w, b = 1 + randn(g, C, scale=0.2), randn(g, C, scale=0.1)
    gh, gs = randn(g, rows, C), randn(g, rows, C)
    xd, yd, ybd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, y, yb, w, b))
    s, h = spf.add_layer_norm(xd, yd, wd, bd, EPS_LN, y_bias=ybd)
    s_saved, _, stats = h.grad_fn.saved_tensors
    torch.autograd.backward([s, h], [gs.cuda(), gh.cuda()])
    assert torch.equal(xd.grad, yd.grad)
    x64, y64, yb64 = x.double(), y.double(), yb.double()
    sref, sb = R.ln_sum(x64, y64, yb64)
    gate("layernorm add", f"{rows} rows s", s, sref, sb, [whole(-yb64.expand(rows, C)), [((0,), -x64[0])]])
    s64 = host(s_saved)
    ln_gates(f"{rows} rows", s64, stats, w.double(), b.double(), h, gh.double(), gs.double(), xd.grad, (wd.grad, bd.grad), 3,
             R.ln_rows_per_wave(rows), ybd.grad)


def test_layer_norm_without_y_at_full_size(env):
    spf, _ = env
    rows, C = 2312, 768
    g = gen(2313)
    x, w, b, gh = randn(g, rows, C) * 2 + 0.5, 1 + randn(g, C, scale=0.2), randn(g, C, scale=0.1), randn(g, rows, C)
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
    h = spf.layer_norm(xd, wd, bd, EPS_LN)
    _, _, stats = h.grad_fn.saved_tensors
    h.backward(gh.cuda())
    ln_gates("layer_norm 2312 rows", x.double(), stats, w.double(), b.double(), h, gh.double(), None, xd.grad, (wd.grad, bd.grad), 3,
             R.ln_rows_per_wave(rows))


# ---------------------------------------------------------------- sample-down
GAMMA, BETA = torch.tensor([1.3, 0.7, 1.1]), torch.tensor([0.1, -0.2, 0.3])
RM0, RV0 = torch.tensor([0.2, -0.1, 0.3]), torch.tensor([0.8, 1.2, 0.9])


def run_sample_down(spf, img, w9, b3, gy, training):
    cw, cb = w9.float().cuda().requires_grad_(True), b3.float().cuda().requires_grad_(True)
    gd, bd = GAMMA.cuda().requires_grad_(True), BETA.cuda().requires_grad_(True)
    rm, rv = RM0.cuda(), RV0.cuda()
    out = spf.sample_down(img.float().cuda(), cw, cb, gd, bd, rm, rv, MOM, EPS, training, (384, 384))
    saved = out.grad_fn.saved_tensors[4].detach().cpu()
    if gy is not None:
        out.backward(gy.float().cuda())
    return out, saved, rm, rv, (cw.grad, cb.grad, gd.grad, bd.grad)


def gate_sd_forward(what, img, w9, b3, out, saved, rm, rv, e, n, ev_scale):
    sums = saved[:27]
    mean, var, inv = R.sd_stats(sums, n, EPS)
    mb, ib, vb = R.sd_stats_bounds(sums, e, n, mean, inv)
    pre = R.sd_pre(img, w9, b3).clamp_min(0)
    vmax = pre.amax((0, 2, 3))
    xp = R.sd_picked(img, 384, 384)
    mean_p, var_p, inv_p = R.sd_stats(R.sd_forward_sums(xp, w9, b3), xp.numel() // 3, EPS)     # over the picked pixels only
    gate("sample_down statistics", what + " mean", saved[27:30], mean, mb, [whole(-vmax / n), whole(mean_p - mean)])
    gate("sample_down statistics", what + " invstd", saved[30:33], inv, ib,
         [whole(inv_p - inv), whole(R.bn_invstd((sums[3:6] - vmax ** 2) / n - mean ** 2, EPS) - inv)])
    # (the unbiased correction n / (n - 1) of running_var is below one float32 rounding at these N: not a usable mutant)
    mk = f32(saved[27:30])
    rm_ref, rv_ref = R.bn_running(RM0.double(), RV0.double(), mk, var, n, MOM)
    rvb = 4 * U * ((1 - MOM) * RV0.double() + MOM * var * n / (n - 1)) + MOM * n / (n - 1) * vb
    gate("sample_down statistics", what + " running mean", rm, rm_ref, 4 * U * ((1 - MOM) * RM0.double().abs() + MOM * mk.abs()),
         [whole(-MOM * vmax / n), whole(R.bn_running(RM0.double(), RV0.double(), mk, var, n, 1 - MOM)[0] - rm_ref)])
    gate("sample_down statistics", what + " running var", rv, rv_ref, rvb,
         [whole(R.bn_running(RM0.double(), RV0.double(), mk, var_p, n, MOM)[1] - rv_ref), whole(-MOM * vmax ** 2 / n)])
    xp = R.sd_picked(img, 384, 384)
    ref, bound = R.sd_out(xp, w9, b3, f32(saved[27:30]), f32(saved[30:33]), GAMMA.double(), BETA.double(), ev_scale)
    gate("sample_down pick", what + " output", out, ref, bound,
         [whole(R.sd_out(xp, w9, b3, f32(mean_p), f32(inv_p), GAMMA.double(), BETA.double())[0] - ref), [((0, 0, slice(None), 5), ref[0, 0, :, 6] - ref[0, 0, :, 5])]])


def gate_sd_backward(what, img, gy, w9, b3, saved, n, grads, ev_scale, saved_ge=None):
    ref, bound, amb = R.sd_backward(img, gy, w9, b3, GAMMA.double(), saved, n, ev_scale=ev_scale)
    mut = dict(picked=R.sd_backward(img, gy, w9, b3, GAMMA.double(), saved, n, n_picked=True, ev_scale=ev_scale)[0],
               s2=R.sd_backward(img, gy, w9, b3, GAMMA.double(), saved, n, drop_s2=True, ev_scale=ev_scale)[0])
    if saved_ge is not None:
        mut["ge"] = R.sd_backward(img, gy, w9, b3, GAMMA.double(), saved_ge, n, mask_ge=True, ev_scale=ev_scale)[0]
    first = "ge" if saved_ge is not None else "s2"
    for key, got in (("gw9", grads[0]), ("gb3", grads[1])):
        gate("sample_down backward", f"{what} {key}", got, ref[key], bound[key],
             [whole(mut[first][key] - ref[key]), whole(mut["picked"][key] - ref[key])])
    gyr = gy.clone()
    gyr[:, :, -1] = 0                                                   # the last output row missing from the sums
    short = R.sd_backward(img, gyr, w9, b3, GAMMA.double(), saved, n, ev_scale=ev_scale)[0]
    dup = R.sd_backward(img, gy, w9, b3, GAMMA.double(), saved, n, drop_dup=True, ev_scale=ev_scale)[0]
    for key, got in (("ggamma", grads[2]), ("gbeta", grads[3])):
        second = dup if img.shape[2] < 384 else R.sd_backward(img, gy * 0.999, w9, b3, GAMMA.double(), saved, n, ev_scale=ev_scale)[0]
        gate("sample_down backward", f"{what} {key}", got, ref[key], bound[key], [whole(short[key] - ref[key]), whole(second[key] - ref[key])])
    if img.shape[2] < 384:
        assert R.ratio(dup["gw9"], ref["gw9"], bound["gw9"]) > 1 and R.ratio(dup["gb3"], ref["gb3"], bound["gb3"]) > 1
    return amb


def test_sample_down_train_dyadic_at_full_size(env):
    """B = 4, 370 x 1226 -> 384 x 384 (14 source rows picked twice) on a dyadic image and weights (k/64, k/16): W x + b is exact under
    any contraction, so the 27 sums over all pixels are exact (assert_array_equal), and pixels planted with W x + b == 0 among the
    picked ones show the mask's strictness (m = v > 0) in sum m, sum m x_c and in d W / d b."""
    spf, _ = env
    g = gen(370)
    w9, b3 = R.dyadic_params(g)
    img = R.plant_zeros(R.dyadic_image(g, 4, 370, 1226), w9, b3, 384, 384, per_channel=300, seed=1)
    gy = torch.randint(-64, 65, (4, 3, 384, 384), generator=g).double() / 64
    pre = R.sd_pre(img, w9, b3)
    assert torch.equal(pre, f32(pre))
    out, saved, rm, rv, grads = run_sample_down(spf, img, w9, b3, gy, True)
    n = img.numel() // 3
    sums = R.sd_forward_sums(img, w9, b3)
    np.testing.assert_array_equal(saved[:27].numpy(), sums.numpy())
    saved_ge = saved.clone()
    saved_ge[:27] = R.sd_forward_sums(img, w9, b3, mask_ge=True)
    assert not torch.equal(saved_ge[6:18], saved[6:18])
    xp = R.sd_picked(img, 384, 384)
    assert int((R.sd_pre(xp, w9, b3) == 0).sum()) >= 600
    gate_sd_forward("dyadic", img, w9, b3, out, saved, rm, rv, torch.zeros(27, dtype=torch.float64), n, 0.0)
    gate_sd_backward("dyadic", img, gy, w9, b3, saved, n, grads, 0.0, saved_ge)


def test_sample_down_train_normal_image_at_full_size(env):
    """B = 4, 900 x 1600 (NuScenes), normal-valued: a pixel whose float64 pre-activation lies within its rounding bound of 0 may take
    either mask; its largest effect is part of every bound, and there are only a handful."""
    spf, _ = env
    g = gen(900)
    img = randn(g, 4, 3, 900, 1600).double()
    w9, b3 = randn(g, 3, 3, scale=0.5).double(), randn(g, 3, scale=0.2).double()
    gy = randn(g, 4, 3, 384, 384).double()
    out, saved, rm, rv, grads = run_sample_down(spf, img, w9, b3, gy, True)
    n = img.numel() // 3
    sums = R.sd_forward_sums(img, w9, b3)
    e, amb = R.sd_forward_sum_bounds(img, w9, b3)
    assert int(amb.sum()) <= 60, amb
    big = int(torch.argmax(R.sd_pre(img, w9, b3)[0, 0].reshape(-1)))
    px = img[0, :, big // 1600, big % 1600]
    v = R.sd_pre(px[None, :, None], w9, b3).reshape(3).clamp_min(0)
    one = torch.cat([v, v * v, (v > 0).double(), ((v > 0).double()[:, None] * px[None]).reshape(9), (v[:, None] * px[None]).reshape(9)])
    # v, v^2, v x_c: gated; m, m x_c: an ambiguous pixel that took the other mask moves them by exactly its whole bound (1, |x_c|),
    # so those are checked as the claim itself -- within the ambiguous pixels' effect -- and the flips are reported
    cont = torch.cat([torch.arange(0, 6), torch.arange(18, 27)])
    gate("sample_down sums", "normal sums", saved[cont], sums[cont], e[cont], [whole(-one[cont]), whole(one[cont])])
    flips = (saved[6:18] - sums[6:18]).abs()
    assert bool((flips <= e[6:18]).all()), (flips, e[6:18])
    NOTES.append(f"900x1600: ambiguous pixels per channel {amb.int().tolist()}, mask flips in sum m {flips[:3].int().tolist()}")
    gate_sd_forward("normal", img, w9, b3, out, saved, rm, rv, e, n, 1.0)
    amb_p = gate_sd_backward("normal", img, gy, w9, b3, saved, n, grads, 1.0)
    assert amb_p <= 20, amb_p


def test_sample_down_eval_at_full_size(env):
    """training=0: the running statistics normalise the picked pixels and stay as they were."""
    spf, _ = env
    g = gen(371)
    img = randn(g, 4, 3, 370, 1226).double()
    w9, b3 = randn(g, 3, 3, scale=0.5).double(), randn(g, 3, scale=0.2).double()
    out, saved, rm, rv, _ = run_sample_down(spf, img, w9, b3, None, False)
    assert torch.equal(rm.cpu(), RM0) and torch.equal(rv.cpu(), RV0)
    inv = R.bn_invstd(RV0.double(), EPS)
    assert torch.equal(saved[27:30], RM0.double())
    n = img.numel() // 3
    batch_mean, _, batch_inv = R.sd_stats(R.sd_forward_sums(img, w9, b3), n, EPS)
    gate("sample_down statistics", "eval invstd", saved[30:33], inv, 4 * R.D * inv, [whole(batch_inv - inv), whole(R.bn_invstd(RV0.double(), 0) - inv)])
    xp = R.sd_picked(img, 384, 384)
    ref, bound = R.sd_out(xp, w9, b3, RM0.double(), f32(saved[30:33]), GAMMA.double(), BETA.double())
    gate("sample_down pick", "eval output", out, ref, bound,
         [whole(R.sd_out(xp, w9, b3, f32(batch_mean), f32(batch_inv), GAMMA.double(), BETA.double())[0] - ref),
          [((0, 0, slice(None), 5), ref[0, 0, :, 6] - ref[0, 0, :, 5])]])
