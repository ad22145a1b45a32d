"""The sparse-convolution kernels (csrc/ftx_spconv.hip) against a float64 reference at the tile shapes they run at.

Every result is compared with a float64 computation on the CPU from the same float32 inputs, per element, under an error bound
rather than a fixed tolerance:

    |got - ref| <= (m + 8) * 2^-24 * R

R is the same computation on |inputs| and m the longest chain of float32 additions into the element.  The fp32 MFMA computes
products exactly, so the bound holds for any summation order with chains of at most m additions:
  * pair GEMM + reduce, scatter form: m = c_in + kvol (the MFMA chain over c_in, then the reduce over the offsets);
  * dense rows: m = c_in (+ 1 with a bias);
  * weight gradient: m = tile_len + tiles of the offset + 16 (a tile's pairs, the KS wave groups, the TL lanes of the ordered reduce
    and their sum).  The worst case over every tiling, 4096 + 64, is too loose to see one pair among the 81 k of a centre offset.
Next to every such comparison the gate is applied to two mutants of the reference -- one pair's contribution removed from the middle
of the largest offset, and that pair credited to the neighbouring offset's weight -- and must reject both.

The layers come from tests/spconv_regimes.py, whose regimes tests/test_spconv_regimes.py checks without a GPU."""
import time

import numpy as np
import pytest
import torch

from tests import spconv_regimes as S
from tests.norm_ref import (U, WORST, check, conv_check, conv_mutants, conv_ref, gen, probe_pair, randn, ratio,  # noqa: F401
                            wgrad_bound_m, wgrad_check, wgrad_mutants, wgrad_ref)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield spf, _lib.load()
    print("\nworst error / bound per kernel: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


# ---------------------------------------------------------------- pair lists
def pair_list(g, sizes, n_src, n_dst):
    """Pair list of the given offset sizes: gather indices with repeats and the last row, distinct destination rows per offset
    (a kernel map joins a row to at most one row per offset).  Returns host (src, dst, koff) and device (src, dst, koff, pos)."""
    kvol = len(sizes)
    assert n_dst >= max(sizes)
    koff = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    src = torch.randint(0, n_src, (int(koff[-1]),), generator=g)
    dst = torch.empty_like(src)
    pos = torch.full((kvol, n_dst), -1, dtype=torch.int32)
    for k, c in enumerate(sizes):
        s = int(koff[k])
        if c == 0:
            continue
        rows = torch.randperm(n_dst, generator=g)[:c]
        dst[s:s + c] = rows
        src[s + c // 2] = n_src - 1                              # the last row
        src[s:s + min(c, 4)] = src[s]                            # a repeated row
        pos[k, rows] = torch.arange(s, s + c, dtype=torch.int32)
    d = dict(src=src.int().cuda(), dst=dst.int().cuda(), koff=koff.int().cuda(), pos=pos.cuda())
    return src, dst, koff, d


def random_sizes(g, n_pairs, kvol):
    w = torch.rand(kvol, generator=g)
    w[0] = 0.0                                                   # an empty offset
    w[kvol // 2] *= 6                                            # a centre offset that dominates, as in a submanifold map
    s = (w / w.sum() * n_pairs).floor().long()
    s[kvol // 2] += n_pairs - int(s.sum())
    return [int(v) for v in s]


def pairs_gemm_raw(spf, L, A, W, w_t, src, koff, n_pairs, co):
    """ftx_spconv_pairs_gemm alone: the per-pair rows before the reduce."""
    tmp = torch.empty((n_pairs, co), dtype=torch.float32, device="cuda")
    kvol = koff.shape[0] - 1
    spf.check(L.ftx_spconv_pairs_gemm(A.data_ptr(), A.shape[0], src.data_ptr(), W.data_ptr(), w_t, koff.data_ptr(), n_pairs, A.shape[1], co,
                                      kvol, tmp.data_ptr(), spf._lib.stream()), "ftx_spconv_pairs_gemm")
    return tmp


# ---------------------------------------------------------------- production shapes
@pytest.fixture(scope="module")
def bench_maps(env):
    """Levels and kernel maps of bench.py's first resident batch, built by the CoordinateManager."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.sparse import CoordinateManager
    from oracle import ft_oracle as O
    c = np.asarray(make_batch([0, 1, 2, 3])["coords"]).astype(np.int32)
    c = c[np.argsort(O.sphash(c))]
    cm = CoordinateManager()
    cm.coords[1] = torch.from_numpy(np.ascontiguousarray(c)).cuda()
    for s in (1, 2, 4, 8):
        cm.kernel_map(2, s, 2)
    for s in (1, 2, 4, 8, 16):
        cm.kernel_map(3, s, 1)
    for s, n in S.BENCH_VOXELS.items():
        assert cm.coords[s].shape[0] == n, (s, cm.coords[s].shape[0])
    return cm


def get_map(cm, spec):
    kind, level = spec
    return cm.kernel_map(3, level, 1) if kind == "subm" else cm.kernel_map(2, level, 2)


@pytest.mark.parametrize("e", S.PRODUCTION, ids=[e["name"] for e in S.PRODUCTION])
def test_production_layer_forward_data_and_weight_gradient(env, bench_maps, e):
    spf, L = env
    t0 = time.time()
    km = get_map(bench_maps, e["map"])
    assert km.n_pairs == e["n_pairs"], (e["name"], km.n_pairs)
    kvol, ca, co, P = km.kvol, e["ca"], e["co"], km.n_pairs
    if e["form"] == "deconv":        # transposed conv on the strided map: coarse rows -> fine rows, one pair per fine row
        src_d, dst_d, n_src, n_dst, pos_f, pos_b = km.pair_out, km.pair_in, km.n_out, km.n_in, None, km.pos
    else:
        src_d, dst_d, n_src, n_dst, pos_f, pos_b = km.pair_in, km.pair_out, km.n_in, km.n_out, km.pos, (None if e["form"] == "down_dgrad" else km.pos_t)
    src, dst, koff = src_d.long().cpu(), dst_d.long().cpu(), km.koff.long().cpu()
    g = gen(len(e["name"]) + ca + co)
    A, W, G = randn(g, n_src, ca), randn(g, kvol, ca, co, scale=(ca * kvol) ** -0.5), randn(g, n_dst, co)
    Ad, Wd, Gd = A.cuda(), W.cuda(), G.cuda()

    assert L.ftx_spconv_gemm_block_cols(co, P, kvol) == e["fwd"] and L.ftx_spconv_gemm_block_cols(ca, P, kvol) == e["dgrad"]
    if pos_f is None:
        out = spf._spconv_direct(Ad, Wd, src_d, dst_d, km.koff, P, n_dst, co, 0)
        conv_check("pairs_gemm_scatter", e["name"] + " forward", out, A, W, src, dst, koff, n_dst)
    else:
        out = spf._spconv_apply(Ad, Wd, src_d, pos_f, km.koff, P, n_dst, co, 0)
        conv_check("pairs_gemm+reduce", e["name"] + " forward", out, A, W, src, dst, koff, n_dst)
    Wt = W.transpose(1, 2)
    if pos_b is None:
        gin = spf._spconv_direct(Gd, Wd, dst_d, src_d, km.koff, P, n_src, ca, 1)
        conv_check("pairs_gemm_scatter", e["name"] + " data gradient", gin, G, Wt, dst, src, koff, n_src)
    else:
        gin = spf._spconv_apply(Gd, Wd, dst_d, pos_b, km.koff, P, n_src, ca, 1)
        conv_check("pairs_gemm+reduce", e["name"] + " data gradient", gin, G, Wt, dst, src, koff, n_src)

    assert S.wgrad_regime(L, P, ca, co, kvol) == e["wgrad"]
    dW = spf._spconv_wgrad(Ad, src_d, Gd, dst_d, km.koff, P)
    wgrad_check(L, "pairs_wgrad", e["name"] + " weight gradient", dW, A, src, G, dst, koff)
    if e["wgrad"][2] == 16 and e["wgrad"][1] >= 832:
        assert torch.equal(spf._spconv_wgrad(Ad, src_d, Gd, dst_d, km.koff, P), dW)     # same bits on a second call
    print(f"\n{e['name']}: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("e", S.DENSE, ids=[e["name"] for e in S.DENSE])
def test_dense_rows_linear_at_full_size(env, e):
    """functional.linear on 81 k rows: output (+ bias), input gradient, dense-mode weight gradient and bias gradient."""
    spf, L = env
    n, ca, co = e["rows"], e["ca"], e["co"]
    g = gen(ca * 1000 + co)
    x, W, b, go = randn(g, n, ca), randn(g, co, ca, scale=ca ** -0.5), randn(g, co), randn(g, n, co)
    assert L.ftx_spconv_gemm_block_cols(co, n, 0) == e["fwd"] and L.ftx_spconv_gemm_block_cols(ca, n, 0) == e["dgrad"]
    assert S.wgrad_regime(L, n, co, ca, 1) == e["wgrad"]
    xd, Wd, bd = x.cuda().requires_grad_(True), W.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = spf.linear(xd, Wd, bd)
    y.backward(go.cuda())
    x64, W64, b64, go64 = x.double(), W.double(), b.double(), go.double()
    r, c = n // 2, ca // 2
    ref = x64 @ W64.T + b64
    bound = (ca + 1 + 8) * U * (x64.abs() @ W64.abs().T + b64.abs())
    check("rows_gemm", e["name"] + " forward", y, ref, bound,
          [[((r,), -x64[r, c] * W64[:, c])], [((r,), x64[r, c] * (W64[:, c + 1] - W64[:, c]))]])
    ref = go64 @ W64
    bound = (co + 8) * U * (go64.abs() @ W64.abs())
    j = co // 2
    check("rows_gemm", e["name"] + " input gradient", xd.grad, ref, bound,
          [[((r,), -go64[r, j] * W64[j])], [((r,), go64[r, j] * (W64[j + 1] - W64[j]))]])
    ref = go64.T @ x64
    length = S.wgrad_tile_len(L, n, co, ca, 1)
    bound = (length + S.cdiv(n, length) + 16 + 8) * U * (go64.abs().T @ x64.abs())
    check("pairs_wgrad(dense)", e["name"] + " weight gradient", Wd.grad, ref, bound,
          [[((slice(None),), -torch.outer(go64[r], x64[r]))], [((slice(None),), torch.outer(go64[r], x64[r + 1] - x64[r]))]])
    ref = go64.sum(0)
    bound = 2 * U * ref.abs() + n * 2.0 ** -52 * go64.abs().sum(0)
    check("colsum", e["name"] + " bias gradient", bd.grad, ref, bound, [[((slice(None),), -go64[r])], [((slice(None),), go64[r + 1] - go64[r])]])


def test_dense_weight_gradient_with_one_reduce_lane(env):
    """Dense mode at 700 rows: three tiles, TL = 1."""
    spf, L = env
    g = gen(700)
    A, G = randn(g, 700, 32), randn(g, 700, 64)
    assert S.wgrad_regime(L, 700, 32, 64, 1)[2] == 1
    got = spf._rows_wgrad(A.cuda(), G.cuda())
    idx = torch.arange(700)
    koff = torch.tensor([0, 700])
    ref = wgrad_check(L, "pairs_wgrad(dense)", "dense 700 rows", got[None], A, idx, G, idx, koff)
    assert ref.shape == (1, 32, 64)


# ---------------------------------------------------------------- every instantiation, synthetic pair lists
GEMM_CASES = [  # (ca, co, n_pairs, columns per block)
    (36, 20, 6000, 32), (4, 32, 6000, 32), (100, 64, 6000, 64), (20, 132, 9000, 64), (20, 96, 6000, 96), (132, 192, 9000, 96),
    (36, 128, 60000, 128), (100, 132, 40000, 128),
]


@pytest.mark.parametrize("w_t", [0, 1])
@pytest.mark.parametrize("ca,co,n_pairs,cols", GEMM_CASES)
def test_pair_gemm_every_column_block(env, ca, co, n_pairs, cols, w_t):
    """NT = 1, 2, 3, 4 with W stored (ca, co) and (co, ca); channel counts that are not multiples of 32 put column tiles outside W
    and (ca % 32 != 0) take the zero-filled reduction path."""
    spf, L = env
    g = gen(ca * 7 + co * 13 + n_pairs + w_t)
    sizes = random_sizes(g, n_pairs, 27)
    n_src, n_dst = 5000, max(sizes) + 17
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    assert L.ftx_spconv_gemm_block_cols(co, n_pairs, 27) == cols
    A = randn(g, n_src, ca)
    Wl = randn(g, 27, ca, co, scale=(ca * 27) ** -0.5)            # logical (kvol, ca, co)
    Ws = Wl.transpose(1, 2).contiguous() if w_t else Wl           # as stored
    out = spf._spconv_apply(A.cuda(), Ws.cuda(), d["src"], d["pos"], d["koff"], n_pairs, n_dst, co, w_t)
    conv_check("pairs_gemm+reduce", f"{ca}->{co} wT={w_t}", out, A, Wl, src, dst, koff, n_dst)


WGRAD_CASES = []
for _i, ((_ms, _ca), (_ns, _cg)) in enumerate([(a, b) for a in S.WGRAD_SIDES.items() for b in S.WGRAD_SIDES.items()]):
    WGRAD_CASES.append((_ca[_i % 2], _cg[(_i // 2) % 2], _ms + _ns))


@pytest.mark.parametrize("ca,cg,sides", WGRAD_CASES)
def test_wgrad_every_instantiation(env, ca, cg, sides):
    """Every (MI, WMG) x (NI, WNG) pair of tile sides (pairs_wgrad_kernel<3,3,1,1> is not reachable: wgrad_config sends (3,1) x (3,1)
    to (2,2) x (3,1))."""
    spf, L = env
    g = gen(ca * 31 + cg)
    n_pairs = 30000
    sizes = random_sizes(g, n_pairs, 27)
    n_src, n_dst = 7000, max(sizes) + 5
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    inst = S.wgrad_config(ca, cg)
    assert inst == (sides if sides != (3, 1, 3, 1) else (2, 2, 3, 1))
    A, G = randn(g, n_src, ca), randn(g, n_dst, cg)
    got = spf._spconv_wgrad(A.cuda(), d["src"], G.cuda(), d["dst"], d["koff"], n_pairs)
    wgrad_check(L, "pairs_wgrad", f"wgrad {ca}x{cg} {inst}", got, A, src, G, dst, koff)


def test_wgrad_four_channels_at_a_long_tile(env):
    """The stem's shape (M tile of 32 rows holding 4 channels) at tiles of >= 832 pairs."""
    spf, L = env
    g = gen(4)
    n_pairs = 1700000
    sizes = [n_pairs // 27] * 26 + [n_pairs - 26 * (n_pairs // 27)]    # no dominant offset: one pair must stay visible in each
    _, length, tl = S.wgrad_regime(L, n_pairs, 4, 32, 27)
    assert length >= 832 and tl == 16
    n_src, n_dst = 90000, max(sizes) + 3
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    A, G = randn(g, n_src, 4), randn(g, n_dst, 32)
    got = spf._spconv_wgrad(A.cuda(), d["src"], G.cuda(), d["dst"], d["koff"], n_pairs)
    wgrad_check(L, "pairs_wgrad", "wgrad 4x32 long tile", got, A, src, G, dst, koff)


@pytest.mark.parametrize("kvol", [27, 8, 5])
@pytest.mark.parametrize("ca,cg", [(36, 20), (100, 132)])
def test_tile_edges_of_the_pair_list(env, kvol, ca, cg):
    """Empty first / middle / last offsets, offsets of 1, 31-33, 127-129 pairs, tile_len - 1, tile_len (one tile: written straight to
    dW[k]) and tile_len + 1 (two tiles: reduced), one offset large enough for TL = 16 (TL = 4 with kvol 5); repeated and last-row gather
    indices.  Forward (pair GEMM + the reduce's kvol 27 / 8 / generic instantiation), data gradient and weight gradient."""
    spf, L = env
    sizes, length = S.edge_sizes(L, ca, cg, kvol)
    n_pairs = sum(sizes)
    _, got_len, tl = S.wgrad_regime(L, n_pairs, ca, cg, kvol)
    assert got_len == length and tl == (4 if kvol == 5 else 16)
    g = gen(kvol * 100 + ca)
    n_src, n_dst = 3001, max(sizes) + 11
    src, dst, koff, d = pair_list(g, sizes, n_src, n_dst)
    A, W, G = randn(g, n_src, ca), randn(g, kvol, ca, cg, scale=(ca * kvol) ** -0.5), randn(g, n_dst, cg)
    out = spf._spconv_apply(A.cuda(), W.cuda(), d["src"], d["pos"], d["koff"], n_pairs, n_dst, cg, 0)
    conv_check("pairs_gemm+reduce", f"edges kvol={kvol} forward", out, A, W, src, dst, koff, n_dst)
    # data gradient: the reduce over the source side (pos_t), W read transposed
    pos_t = torch.full((kvol, n_src), -1, dtype=torch.int32)
    # a source row may be gathered by several pairs of one offset here, which a kernel map never does: reduce only over a map-like
    # subset, one pair per (offset, source row) -- the first -- and compare with the reference over the same subset
    keep = torch.zeros(n_pairs, dtype=torch.bool)
    for k in range(kvol):
        s, e = int(koff[k]), int(koff[k + 1])
        seen = set()
        for p in range(s, e):
            i = int(src[p])
            if i not in seen:
                seen.add(i)
                keep[p] = True
                pos_t[k, i] = p
    gin = spf._spconv_apply(G.cuda(), W.cuda(), d["dst"], pos_t.cuda(), d["koff"], n_pairs, n_src, ca, 1)
    ks = torch.searchsorted(koff[1:], torch.nonzero(keep)[:, 0], right=True)
    koff_keep = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(ks, minlength=kvol), 0)])
    conv_check("pairs_gemm+reduce", f"edges kvol={kvol} data gradient", gin, G, W.transpose(1, 2), dst[keep], src[keep], koff_keep, n_src)
    dW = spf._spconv_wgrad(A.cuda(), d["src"], G.cuda(), d["dst"], d["koff"], n_pairs)
    ref = wgrad_check(L, "pairs_wgrad", f"edges kvol={kvol} weight gradient", dW, A, src, G, dst, koff)
    empty = [k for k, c in enumerate(sizes) if c == 0]
    assert empty and bool((dW[empty] == 0).all()) and bool((ref[empty] == 0).all())


# ---------------------------------------------------------------- same bits under another tiling
def test_pair_gemm_rows_do_not_depend_on_the_column_split(env):
    """A column split changes no sum: the pair rows of a prefix of the list, alone (64-column blocks) and as part of the whole list
    (128-column blocks), are the same bits."""
    spf, L = env
    g = gen(99)
    ca, co, n_pairs, n_pre = 64, 128, 60000, 20000
    sizes = random_sizes(g, n_pairs, 27)
    src, dst, koff, d = pair_list(g, sizes, 4000, max(sizes) + 1)
    koff_pre = koff.clamp(max=n_pre)
    assert L.ftx_spconv_gemm_block_cols(co, n_pairs, 27) == 128 and L.ftx_spconv_gemm_block_cols(co, n_pre, 27) == 64
    A, W = randn(g, 4000, ca).cuda(), randn(g, 27, ca, co, scale=0.02).cuda()
    for w_t, Wx in ((0, W), (1, W.transpose(1, 2).contiguous())):
        whole = pairs_gemm_raw(spf, L, A, Wx, w_t, d["src"], d["koff"], n_pairs, co)
        pre = pairs_gemm_raw(spf, L, A, Wx, w_t, d["src"][:n_pre].contiguous(), koff_pre.int().cuda(), n_pre, co)
        assert torch.equal(whole[:n_pre], pre), w_t


def test_output_stationary_conv_is_bit_identical_at_full_size(env, bench_maps):
    """ftx_spconv_ostat against pair GEMM + reduce on the level-1 map of the benched batch (81 k rows, 383 k pairs): forward and the
    mirrored data gradient."""
    spf, L = env
    km = bench_maps.kernel_map(3, 1, 1)
    assert km.n_out == S.BENCH_VOXELS[1] and spf.ostat_supported(32, 32, 27, rows=km.n_out)
    g = gen(32)
    x, w, go = randn(g, km.n_in, 32).cuda(), randn(g, 27, 32, 32, scale=0.03).cuda(), randn(g, km.n_out, 32).cuda()
    ref = spf._spconv_apply(x, w, km.pair_in, km.pos, km.koff, km.n_pairs, km.n_out, 32, 0)
    assert torch.equal(spf._spconv_ostat(x, w, km.nbr, km.n_out, 32, 0, 0), ref)
    ref_g = spf._spconv_apply(go, w, km.pair_out, km.pos_t, km.koff, km.n_pairs, km.n_in, 32, 1)
    assert torch.equal(spf._spconv_ostat(go, w, km.nbr, km.n_in, 32, 1, 1), ref_g)


# ---------------------------------------------------------------- Conv + BatchNorm, fused, at full size
def test_fused_conv_batchnorm_at_full_size(env, bench_maps):
    """conv_bn_train on the 192 -> 128 layer of level 4 against a float64 conv followed by a float64 BatchNorm: the convolution output
    the node keeps for its backward, the batch statistics and running statistics, the output, and the gradients of the BatchNorm
    parameters, of the input and of the weight.  The BatchNorm stages are compared with float64 BatchNorm of the node's own convolution
    output (which is itself gated against the float64 convolution), so that each bound covers one stage."""
    spf, L = env
    km = bench_maps.kernel_map(3, 4, 1)
    ca, co, kvol, n = 192, 128, 27, km.n_out
    assert km.n_pairs == S.BENCH_SUBM_PAIRS[4]
    g = gen(192)
    A, W = randn(g, n, ca), randn(g, kvol, ca, co, scale=(ca * kvol) ** -0.5)
    gam, bet, gy = torch.rand(co, generator=g).float() + 0.5, randn(g, co), randn(g, n, co)
    src, dst, koff = km.pair_in.long().cpu(), km.pair_out.long().cpu(), km.koff.long().cpu()
    Ad, Wd = A.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
    gd, bd = gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
    rm, rv = torch.zeros(co, device="cuda"), torch.ones(co, device="cuda")
    mom, eps = 0.1, 1e-5
    y = spf.conv_bn_train(Ad, Wd, km, False, gd, bd, rm, rv, mom, eps)
    _, _, x_gpu, _, _, _, stats = y.grad_fn.saved_tensors
    y.backward(gy.cuda())

    # the convolution output
    conv_check("pairs_gemm+reduce_stats", "conv output", x_gpu, A, W, src, dst, koff, n)
    x = x_gpu.detach().cpu().double()
    # batch statistics (float64 sums of the float32 output, rounded to float32) and the running statistics
    mu = x.mean(0)
    var = (x * x).mean(0) - mu * mu
    var_b = ((x - mu) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var_b + eps)
    r = int(torch.argmax((x - mu).abs().sum(1)))
    drop_mu = (mu * n - x[r]) / (n - 1) - mu
    st = stats.cpu()
    check("bn statistics", "batch mean", st[0], mu, 2 * U * mu.abs() + 1e-12 * x.abs().mean(0),
          [[((slice(None),), drop_mu)], [((slice(None),), (x[r] - mu) / n)]])
    iv_bound = 2 * U * invstd + invstd ** 3 * 1e-12 * (x * x).mean(0)
    drop_var = ((x * x).sum(0) - x[r] ** 2) / (n - 1) - ((mu * n - x[r]) / (n - 1)) ** 2
    check("bn statistics", "batch invstd", st[1], invstd, iv_bound,
          [[((slice(None),), 1.0 / torch.sqrt(drop_var + eps) - invstd)], [((slice(None),), 1.0 / torch.sqrt(var_b * n / (n - 1) + eps) - invstd)]])
    rm_ref, rv_ref = mom * mu, (1 - mom) + mom * var_b * n / (n - 1)
    check("bn statistics", "running mean", rm, rm_ref, 4 * U * rm_ref.abs() + 1e-12,
          [[((slice(None),), mom * drop_mu)], [((slice(None),), (1 - mom) * mu)]])
    check("bn statistics", "running var", rv, rv_ref, 4 * U * rv_ref.abs(),
          [[((slice(None),), -mom * var_b / (n - 1))], [((slice(None),), mom * (drop_var - var_b) * n / (n - 1))]])
    assert float((var - var_b).abs().max()) < 1e-9

    # output: y = (x - mean) * invstd * gamma + beta in float32 from float32 mean / invstd
    g64, b64 = gam.double(), bet.double()
    xh = (x - mu) * invstd
    ref = xh * g64 + b64
    bound = 8 * U * (g64.abs() * invstd * (x.abs() + mu.abs()) + b64.abs())
    check("bn apply", "output", y, ref, bound,
          [[((r,), -xh[r] * g64)], [((r,), (x[r - 1] - x[r]) * invstd * g64)]])
    # BatchNorm parameter gradients (float64 sums) and the gradient into the convolution output
    gy64 = gy.double()
    dbeta, dgamma = gy64.sum(0), (gy64 * xh).sum(0)
    check("bn backward", "d beta", bd.grad, dbeta, 2 * U * dbeta.abs() + n * 2.0 ** -52 * gy64.abs().sum(0),
          [[((slice(None),), -gy64[r])], [((slice(None),), gy64[r - 1] - gy64[r])]])
    gx_err = (gy64.abs() * (xh.abs() + invstd * mu.abs())).sum(0)
    check("bn backward", "d gamma", gd.grad, dgamma, 8 * U * gx_err + 2 * U * dgamma.abs(),
          [[((slice(None),), -gy64[r] * xh[r])], [((slice(None),), (gy64[r - 1] - gy64[r]) * xh[r])]])
    gx = g64 * invstd * (gy64 - dbeta / n - xh * dgamma / n)
    E_gx = 16 * U * g64.abs() * invstd * (gy64.abs() + dbeta.abs() / n + (xh.abs() + invstd * mu.abs()) * dgamma.abs() / n)
    # input gradient: data gradient of gx through the pair GEMM + reduce; bound = the gate on gx plus the error carried in by gx
    Wt = W.double().transpose(1, 2)
    ref = conv_ref(gx, Wt, dst, src, koff, n)
    bound = (co + kvol + 8) * U * conv_ref(gx.abs(), Wt.abs(), dst, src, koff, n) + conv_ref(E_gx, Wt.abs(), dst, src, koff, n)
    check("pairs_gemm+reduce", "conv_bn input gradient", Ad.grad, ref, bound, conv_mutants(gx, Wt, dst, src, koff))
    wgrad_check(L, "pairs_wgrad", "conv_bn weight gradient", Wd.grad, A, src, gx, dst, koff, extra=E_gx)
