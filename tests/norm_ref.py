"""float64 references and assertion gates for the normalisation kernels -- BatchNorm (csrc/ftx_bn.hip), add + LayerNorm
(csrc/ftx_layernorm.hip), the fused sample-down (csrc/ftx_sampledown.hip) -- and the sparse-convolution gates they share with
tests/test_spconv_regimes_gpu.py.  Used by tests/test_norm_host.py (CPU) and tests/test_norm_fullsize_gpu.py.

Every gate is |got - ref| <= bound per element, with ref evaluated in float64 from the float32 inputs and the bound derived from the
rounding steps the kernel takes (U = 2^-24 per float32 rounding, D = 2^-53 per float64 one).  The gates are stage-wise: the reference
of a stage starts from the kernel's own float32 output of the stage before it (statistics, then apply, then backward), so each bound
covers one stage.  check() applies the gate to the kernel result and to two planted mutants of the reference, which it must reject.

The references take float64 CPU tensors; the mutation switches (drop_row, unbiased=False, ...) are the planted mistakes the host
tests show every gate rejects."""
import torch

from oracle import ft_oracle as O
from tests import spconv_regimes as S

U = 2.0 ** -24
D = 2.0 ** -53
WORST = {}      # kernel -> worst ratio of error to bound, printed at the end of a GPU module


def ratio(got, ref, bound):
    """max |got - ref| / bound (float64); an element whose bound is 0 must match exactly."""
    d = (got.double() - ref).abs()
    if bool(((bound <= 0) & (d > 0)).any()):
        return float("inf")
    r = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.zeros_like(d))
    return float(r.max()) if r.numel() else 0.0


def check(kernel, what, got, ref, bound, mutants):
    """The gate on got, and on each mutant of the reference: a mutant is a list of (index, delta) parts, ref[index] + delta."""
    got = got.detach().cpu()
    ref, bound = ref.detach(), bound.detach()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    r = ratio(got, ref, bound)
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    assert r <= 1.0, f"{what}: error is {r:.3g} x the bound"
    assert len(mutants) == 2
    for i, parts in enumerate(mutants):
        assert any(ratio(ref[ix] + dl, ref[ix], bound[ix]) > 1.0 for ix, dl in parts), f"{what}: the gate accepts mutant {i}"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).float()


# ---------------------------------------------------------------- float64 references
def conv_ref(A, W, src, dst, koff, n_dst):
    """out[dst[p]] += A[src[p]] @ W[k(p)], one offset at a time (W oriented (kvol, c_in, c_out))."""
    out = torch.zeros(n_dst, W.shape[2], dtype=torch.float64)
    for k in range(W.shape[0]):
        s, e = int(koff[k]), int(koff[k + 1])
        if e > s:
            out.index_add_(0, dst[s:e], A[src[s:e]] @ W[k])
    return out


def wgrad_ref(A, ia, G, ig, koff):
    kvol = koff.shape[0] - 1
    out = torch.zeros(kvol, A.shape[1], G.shape[1], dtype=torch.float64)
    for k in range(kvol):
        s, e = int(koff[k]), int(koff[k + 1])
        if e > s:
            out[k] = A[ia[s:e]].T @ G[ig[s:e]]
    return out


def probe_pair(koff):
    """(pair in the middle of the largest offset, its offset, the neighbouring offset)."""
    cnt = (koff[1:] - koff[:-1])
    k = int(torch.argmax(cnt))
    kn = k + 1 if k + 1 < cnt.shape[0] else k - 1
    return int(koff[k]) + int(cnt[k]) // 2, k, kn


def conv_mutants(A, W, src, dst, koff):
    p, k, kn = probe_pair(koff)
    a, o = A[src[p]], int(dst[p])
    c = a @ W[k]
    return [[((o,), -c)], [((o,), a @ W[kn] - c)]]


def wgrad_mutants(A, ia, G, ig, koff):
    p, k, kn = probe_pair(koff)
    # of the 64 pairs around the middle, the one with the largest contribution
    lo, hi = max(int(koff[k]), p - 32), min(int(koff[k + 1]) - 1, p + 32)
    w = torch.arange(lo, hi)
    p = int(w[torch.argmax(A[ia[w]].abs().amax(1) * G[ig[w]].abs().amax(1))])
    outer = torch.outer(A[ia[p]], G[ig[p]])
    if koff.shape[0] == 2:    # one offset (dense rows): the pair credited with the next pair's G row instead
        return [[((k,), -outer)], [((k,), torch.outer(A[ia[p]], G[ig[p + 1]]) - outer)]]
    return [[((k,), -outer)], [((k,), -outer), ((kn,), outer)]]


def conv_check(kernel, what, got, A, W, src, dst, koff, n_dst):
    """Pair GEMM (+ reduce): float64 reference, bound with m = c_in + kvol, and the two mutants."""
    A, W = A.double(), W.double()
    ref = conv_ref(A, W, src, dst, koff, n_dst)
    bound = (W.shape[1] + W.shape[0] + 8) * U * conv_ref(A.abs(), W.abs(), src, dst, koff, n_dst)
    check(kernel, what, got, ref, bound, conv_mutants(A, W, src, dst, koff))
    return ref


def wgrad_bound_m(lib, koff, ca, cg):
    """Longest addition chain into dW[k] per offset for the weight gradient's tiling (csrc/ftx_spconv_common.h, spconv_wgrad_tile_len
    and wgrad_reduce_kernel): tile_len + tiles of the offset + 16."""
    kvol = koff.shape[0] - 1
    n = int(koff[-1])
    length = S.wgrad_tile_len(lib, n, ca, cg, kvol)
    tiles = (koff[1:] - koff[:-1] + length - 1) // length
    return (length + tiles + 16).double().view(kvol, 1, 1)


def wgrad_check(lib, kernel, what, got, A, ia, G, ig, koff, extra=None):
    """Weight gradient: float64 reference, bound with m = wgrad_bound_m, and the two mutants.  `extra`: a bound on the error G itself
    carries (G computed in float32 by an earlier kernel), added to the bound as sum over pairs of |A| * extra."""
    A, G = A.double(), G.double()
    ref = wgrad_ref(A, ia, G, ig, koff)
    m = wgrad_bound_m(lib, koff, A.shape[1], G.shape[1])
    bound = (m + 8) * U * wgrad_ref(A.abs(), ia, G.abs(), ig, koff)
    if extra is not None:
        bound = bound + wgrad_ref(A.abs(), ia, extra, ig, koff)
    check(kernel, what, got, ref, bound, wgrad_mutants(A, ia, G, ig, koff))
    return ref


def f32(t):
    """t rounded to float32, as float64."""
    return t.float().double()


def row_parts(delta, r):
    """A mutant that changes row r of the reference by delta (a vector)."""
    return [((r,), delta)]


def whole(delta):
    """A mutant that changes the whole reference by delta (same shape)."""
    return [((slice(None),), delta)]


# ================================================================ BatchNorm1d over rows (csrc/ftx_bn.hip)
def bn_stats(x, drop_row=None):
    """Batch mean and biased variance per column of x (n, c); drop_row: that row left out (a planted mistake)."""
    if drop_row is not None:
        x = torch.cat([x[:drop_row], x[drop_row + 1:]])
    mu = x.mean(0)
    return mu, ((x - mu) ** 2).mean(0)


def bn_invstd(var, eps):
    return 1.0 / torch.sqrt(var + eps)


def bn_stats_bounds(x, mean, invstd):
    """Bounds on the float32 mean and invstd a statistics pass stores.  The float64 column sums of x and x*x (products exact) are off
    by at most n D sum|x| and n D sum x^2; the variance sum/n - mean^2 by 4 n D mean(x^2); invstd moves by invstd^3 / 2 per unit of
    variance; each value is rounded to float32 once."""
    n = x.shape[0]
    return 2 * U * mean.abs() + 2 * n * D * x.abs().mean(0), 2 * U * invstd + 4 * n * D * invstd ** 3 * (x * x).mean(0)


def bn_running(rm0, rv0, mean_k, var, n, momentum, unbiased=True):
    """running_mean / running_var after one training forward: (1 - m) r + m * stat with the kernel's float32 mean and the float64
    variance, unbiased (n / (n - 1)) for running_var; unbiased=False is a planted mistake."""
    v = var * n / (n - 1) if unbiased and n > 1 else var
    return (1 - momentum) * rm0 + momentum * mean_k, (1 - momentum) * rv0 + momentum * v


def bn_running_bounds(rm0, rv0, mean_k, var, x, momentum):
    """Four float32 roundings (1 - m, two products, the sum) on each; running_var also carries the float64 variance's error."""
    n = x.shape[0]
    v = var * n / (n - 1)
    return (4 * U * ((1 - momentum) * rm0.abs() + momentum * mean_k.abs()),
            4 * U * ((1 - momentum) * rv0.abs() + momentum * v) + momentum * n / (n - 1) * 4 * n * D * (x * x).mean(0))


def bn_apply(x, mean, invstd, gamma, beta, residual=None, relu=False, ulps=4):
    """y = relu?((x - mean) * invstd * gamma + beta (+ residual)) -> (y, pre-activation, bound).  The training apply (bn_affine) rounds
    x - mean, the product with invstd and the fma with gamma and beta, then the residual add: 4U of the absolute terms bounds the float32
    pre-activation (ulps=6 for the eval kernel, which also rounds invstd and leaves contraction to the compiler).  ReLU is
    1-Lipschitz, so the bound holds for y whatever side of 0 the float32 pre-activation falls on."""
    pre = (x - mean) * invstd * gamma + beta
    R = (x - mean).abs() * invstd * gamma.abs() + beta.abs()
    if residual is not None:
        pre = pre + residual
        R = R + residual.abs()
    return (pre.clamp_min(0) if relu else pre), pre, ulps * U * R


def bn_eval(x, rm, rv, eps, gamma, beta, residual=None, relu=False):
    """bn_apply_eval_kernel: invstd = float32(1 / sqrt(running_var + eps)) in float64, then as bn_apply with six float32 roundings."""
    return bn_apply(x, rm, bn_invstd(rv, eps), gamma, beta, residual, relu, ulps=6)


def bn_backward(gy, x, mean, invstd, gamma, mask=None, drop_row=None):
    """Training-mode BatchNorm backward from the kernel's float32 mean / invstd -> (dict(dy, dbeta, dgamma, gx), dict of bounds).

    mask is the ReLU mask (bool, None without ReLU), an ARGUMENT: the tests pass the kernel's own y > 0, so that a float64
    pre-activation within rounding of 0 cannot flip the reference.  dy = gy * mask is also the residual gradient (exact).
    Bounds: d beta = float32 of a float64 sum of dy; d gamma also rounds xhat = (x - mean) * invstd twice in float32 (2U of each
    term); gx = gamma * invstd * (dy - f32(d beta) / n - xhat * f32(d gamma) / n) with float32(1 / n) and at most eight more
    float32 roundings along any term: 12U of the absolute terms, plus the sums' float64 error.  drop_row: one row left out of the two
    sums (a planted mistake)."""
    dy = gy if mask is None else gy * mask
    n = x.shape[0]
    xh = (x - mean) * invstd
    dyx = dy * xh
    keep = slice(None) if drop_row is None else torch.arange(n) != drop_row
    S0, S1 = dy[keep].sum(0), dyx[keep].sum(0)
    gx = gamma * invstd * (dy - S0 / n - xh * S1 / n)
    A0, A1 = dy.abs().sum(0), dyx.abs().sum(0)
    b = dict(dbeta=2 * U * S0.abs() + 2 * n * D * A0,
             dgamma=2 * U * S1.abs() + (3 * U + 2 * n * D) * A1,
             gx=gamma.abs() * invstd * (12 * U * (dy.abs() + S0.abs() / n + xh.abs() * (S1.abs() + A1) / n) + 2 * D * (A0 + xh.abs() * A1)))
    return dict(dy=dy, dbeta=S0, dgamma=S1, gx=gx), b


# ================================================================ add + LayerNorm over token rows (csrc/ftx_layernorm.hip)
def ln_sum(x, y=None, y_bias=None):
    """s = x + (y + y_bias) -> (s, bound): two float32 roundings."""
    if y is None:
        return x, torch.zeros_like(x)
    t, R = (y, y.abs()) if y_bias is None else (y + y_bias, y.abs() + y_bias.abs())
    return x + t, 3 * U * (x.abs() + R)


def ln_stats(s, eps, mean_k=None, drop_col=None, ddof=0):
    """Per-row mean of s and rstd = 1 / sqrt(sum((s - mean_k)^2) / (C - ddof) + eps), centred on the kernel's float32 mean mean_k (its
    second pass uses its own mean; None: the float64 mean).  drop_col: both sums missing that column; ddof=1: the variance over C - 1
    (planted mistakes)."""
    C = s.shape[1]
    keep = torch.ones(C, dtype=torch.bool)
    if drop_col is not None:
        keep[drop_col] = False
    mean = s[:, keep].sum(1) / C
    mk = mean if mean_k is None else mean_k
    return mean, 1.0 / torch.sqrt(((s[:, keep] - mk[:, None]) ** 2).sum(1) / (C - ddof) + eps)


def ln_stats_bounds(s, rstd, vpl):
    """The kernel sums a row in float32 over chains of at most VPL + 8 additions (per lane, (x + y) + (z + w) per float4 and VPL float4
    in a row, then a 6-level butterfly) and multiplies by float32(1 / C): the mean is within (VPL + 12) U mean|s|.  The squares add a
    subtraction and a product (3U each) to the same chain, + eps one more, and rsqrtf (1 ulp, 2U) rounds the root: rstd within
    (VPL + 16) U rstd."""
    return (vpl + 12) * U * s.abs().mean(1), (vpl + 16) * U * rstd


def ln_apply(s, mean_k, rstd_k, gamma, beta):
    """h = (s - mean) * rstd * gamma + beta from the kernel's float32 mean / rstd -> (h, bound): four float32 roundings."""
    c = s - mean_k[:, None]
    return c * rstd_k[:, None] * gamma + beta, 4 * U * (c.abs() * rstd_k[:, None] * gamma.abs() + beta.abs())


def ln_backward(gh, gs, s, gamma, mean_k, rstd_k, vpl, rows_per_wave, add_gs=True):
    """Backward of h = LayerNorm(s) (+ the residual gradient gs) from the kernel's float32 mean / rstd
    -> (dict(gx, dgamma, dbeta), dict of bounds).

    gx = rstd * (gy - c1 - xhat * c2) + gs, gy = gh * gamma, c1 / c2 the row means of gy and gy * xhat: the kernel rounds xhat twice and
    gy once, sums c1 / c2 like the forward's mean ((VPL + 14) U of the row's absolute terms), and rounds the row expression at most five
    more times: (VPL + 15) U overall, and 2U of |gs| for its add.  d gamma / d beta: each wave sums its rows_per_wave rows in float32
    (products 3U), the rest in float64, one float32 rounding.  add_gs=False: gs not added (a planted mistake)."""
    r = rstd_k[:, None]
    xh = (s - mean_k[:, None]) * r
    gy = gh * gamma
    c1 = gy.mean(1, keepdim=True)
    c2 = (gy * xh).mean(1, keepdim=True)
    gx = r * (gy - c1 - xh * c2)
    gb = r * (vpl + 15) * U * (gy.abs() + gy.abs().mean(1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(1, keepdim=True))
    if gs is not None:
        gb = gb + 2 * U * gs.abs()
        if add_gs:
            gx = gx + gs
    dgamma, dbeta = (gh * xh).sum(0), gh.sum(0)
    k = rows_per_wave
    return dict(gx=gx, dgamma=dgamma, dbeta=dbeta), dict(
        gx=gb, dgamma=(k + 4) * U * (gh * xh).abs().sum(0) + 2 * U * dgamma.abs(), dbeta=(k + 1) * U * gh.abs().sum(0) + 2 * U * dbeta.abs())


def ln_colsum(gx, rows_per_wave):
    """d y_bias = the column sums of the kernel's own gx -> (ref, bound): float32 within a wave's rows, float64 after."""
    ref = gx.sum(0)
    return ref, (rows_per_wave + 1) * U * gx.abs().sum(0) + 2 * U * ref.abs()


def ln_rows_per_wave(rows):
    """ln_rows_per_block(rows) / 4 waves: 1, 2, 4 rows per wave for < 1024, < 2048, >= 2048 rows."""
    return 4 if rows >= 2048 else (2 if rows >= 1024 else 1)


# ================================================================ sample-down: Conv1x1(3->3) -> ReLU -> BatchNorm2d -> nearest pick
def dyadic_image(g, B, H, W):
    """Values k/64 in [-2, 2]: with weights k/16, W x + b is exact in float32 under any contraction."""
    return torch.randint(-128, 129, (B, 3, H, W), generator=g).double() / 64


def dyadic_params(g):
    w9 = torch.randint(-16, 17, (3, 3), generator=g).double() / 16
    w9.diagonal().fill_(0.5)
    return w9, torch.tensor([-3.0, 5.0, -1.0], dtype=torch.float64) / 16


def plant_zeros(img, w9, b3, oh, ow, per_channel=40, seed=0):
    """At picked pixels, x = e_o * (-b_o / W_oo) so that channel o's pre-activation is exactly 0."""
    rows, cols = sd_pick_index(img.shape[2], img.shape[3], oh, ow)
    g = torch.Generator().manual_seed(seed)
    for o in range(3):
        for _ in range(per_channel):
            bi = int(torch.randint(0, img.shape[0], (1,), generator=g))
            r, c = int(rows[int(torch.randint(0, oh, (1,), generator=g))]), int(cols[int(torch.randint(0, ow, (1,), generator=g))])
            img[bi, :, r, c] = 0
            img[bi, o, r, c] = -b3[o] / w9[o, o]
    assert float(((sd_pre(img, w9, b3) == 0) & (img.abs().sum(1, keepdim=True) > 0)).sum()) >= 3 * per_channel
    return img


def sd_pick_index(H, W, oh, ow):
    """Source row and column of every output pixel of nn.Upsample((oh, ow)) (nearest, float32 scale)."""
    return torch.from_numpy(O.nearest_src_index(oh, H)), torch.from_numpy(O.nearest_src_index(ow, W))


def sd_pre(img, w9, b3):
    """The 1x1 convolution's output (B, 3, ...) in float64."""
    return torch.einsum("oc,bc...->bo...", w9, img) + b3.view([1, 3] + [1] * (img.dim() - 2))


def sd_forward_sums(img, w9, b3, mask_ge=False):
    """The 27 float64 sums of the statistics pass over ALL pixels: v (3), v^2 (3), m (3), m * x_c (9, o-major), v * x_c (9), with
    v = relu(W x + b) and m = (v > 0); mask_ge: m = (W x + b >= 0) (a planted mistake)."""
    pre = sd_pre(img, w9, b3)
    v = pre.clamp_min(0)
    m = ((pre >= 0) if mask_ge else (pre > 0)).double()
    dims = [0] + list(range(2, img.dim()))
    return torch.cat([v.sum(dims), (v * v).sum(dims), m.sum(dims), torch.einsum("bo...,bc...->oc", m, img).reshape(9),
                      torch.einsum("bo...,bc...->oc", v, img).reshape(9)])


def sd_forward_sum_bounds(img, w9, b3):
    """Bounds on the 27 sums when the float32 pre-activation is off by up to ev = 4U (|W| |x| + |b|) (three products, three adds) ->
    (bounds, ambiguous pixels per channel).  A pixel with |W x + b| <= ev may take either mask: it moves sum m by 1 and sum m x_c by
    |x_c|; v and v * x_c move by ev and ev |x_c| (ReLU is 1-Lipschitz); the float64 sums add 2 N D of their absolute terms."""
    pre = sd_pre(img, w9, b3)
    v = pre.clamp_min(0)
    ev = 4 * U * sd_pre(img.abs(), w9.abs(), b3.abs())
    amb = (pre.abs() <= ev).double()
    ax = img.abs()
    dims = [0] + list(range(2, img.dim()))
    n = pre.numel() // 3
    e = torch.cat([ev.sum(dims) + 2 * n * D * v.sum(dims), (2 * v * ev + ev * ev).sum(dims) + 2 * n * D * (v * v).sum(dims), amb.sum(dims),
                   torch.einsum("bo...,bc...->oc", amb, ax).reshape(9) + 2 * n * D * torch.einsum("bo...,bc...->oc", (pre > 0).double(), ax).reshape(9),
                   torch.einsum("bo...,bc...->oc", ev, ax).reshape(9) + 2 * n * D * torch.einsum("bo...,bc...->oc", v, ax).reshape(9)])
    return e, amb.sum(dims)


def sd_stats(sums, n, eps):
    """mean, biased variance and invstd of the three channels from the sums, as sd_finalize_fwd_kernel forms them (float64)."""
    mean = sums[0:3] / n
    var = (sums[3:6] / n - mean * mean).clamp_min(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def sd_stats_bounds(sums, e, n, mean, invstd):
    """Bounds on saved mean / invstd (and on the variance) from the bounds e on the sums and a few float64 roundings."""
    e_var = e[3:6] / n + 2 * mean.abs() * e[0:3] / n + (e[0:3] / n) ** 2 + 8 * D * (sums[3:6] / n + mean * mean)
    return e[0:3] / n + 2 * D * mean.abs(), invstd ** 3 / 2 * e_var + 4 * D * invstd, e_var


def sd_picked(img, oh, ow):
    """The picked pixels (B, 3, oh, ow) of img (duplicates repeated)."""
    rows, cols = sd_pick_index(img.shape[2], img.shape[3], oh, ow)
    return img[:, :, rows][:, :, :, cols]


def sd_out(xp, w9, b3, mean_k, invstd_k, gamma, beta, ev_scale=1.0):
    """The output at the picked pixels from the kernel's float32 mean / invstd -> (out, bound): relu(W x + b) off by at most
    ev_scale * 4U (|W| |x| + |b|) (0 for dyadic inputs, where every step is exact), then four float32 roundings."""
    v = sd_pre(xp, w9, b3).clamp_min(0)
    ev = ev_scale * 4 * U * sd_pre(xp.abs(), w9.abs(), b3.abs())
    c = v - mean_k.view(1, 3, 1, 1)
    s = (invstd_k * gamma).view(1, 3, 1, 1)
    return c * s + beta.view(1, 3, 1, 1), ev * s.abs() + 4 * U * (c.abs() * s.abs() + beta.abs().view(1, 3, 1, 1))


def sd_backward(img, gy, w9, b3, gamma, saved, n, mask_ge=False, n_picked=False, drop_s2=False, drop_dup=False, ev_scale=1.0):
    """The BatchNorm2d gradients of sd_finalize_bwd_kernel in closed form, from the forward's saved float64 values (the 27 sums, mean,
    invstd) and sums over the picked pixels (a source row picked twice counts twice):
        S1 = sum dy, S2 = sum dy xhat, Dm = sum dy m, A_oc = sum dy m x_c,     xhat = (v - mean) invstd
        d beta = S1, d gamma = S2,
        d b_o = g is (Dm - S1 / N sum m - S2 / N is (sum v - mean sum m)),   d W_oc likewise with A_oc, sum m x_c, sum v x_c,
    N = every pixel.  -> (dict(gw9, gb3, ggamma, gbeta), dict of bounds).  Planted mistakes: mask_ge (m = (W x + b >= 0)), n_picked
    (N = picked pixels), drop_s2 (the S2 term dropped), drop_dup (the second pick of a duplicated source row dropped).

    Bounds: the kernel forms xhat in float32 from float32(mean), float32(invstd); a picked pixel within ev of 0 may take either mask
    (ev as in sd_out); the float64 sums and formula add a few D of their absolute terms; one float32 rounding."""
    B, _, oh, ow = gy.shape
    rows, _ = sd_pick_index(img.shape[2], img.shape[3], oh, ow)
    xp = sd_picked(img, oh, ow)
    if drop_dup:
        first = torch.ones(oh, dtype=torch.float64)
        first[1:][rows[1:] == rows[:-1]] = 0
        gy = gy * first.view(1, 1, oh, 1)
    pre = sd_pre(xp, w9, b3)
    v = pre.clamp_min(0)
    m = ((pre >= 0) if mask_ge else (pre > 0)).double()
    mean, inv = saved[27:30].view(1, 3, 1, 1), saved[30:33].view(1, 3, 1, 1)
    xh = (v - mean) * inv
    dims = (0, 2, 3)
    S1, S2, Dm = gy.sum(dims), (gy * xh).sum(dims), (gy * m).sum(dims)
    A = torch.einsum("bohw,bchw->oc", gy * m, xp)
    N = B * oh * ow if n_picked else n
    inv3, mean3 = saved[30:33], saved[27:30]
    sum_v, sum_m, mx, vx = saved[0:3], saved[6:9], saved[9:18].view(3, 3), saved[18:27].view(3, 3)
    t2 = torch.zeros(3, dtype=torch.float64) if drop_s2 else S2 / N * inv3
    gi = gamma * inv3
    gb3 = gi * (Dm - S1 / N * sum_m - t2 * (sum_v - mean3 * sum_m))
    gw9 = gi[:, None] * (A - (S1 / N)[:, None] * mx - t2[:, None] * (vx - mean3[:, None] * mx))

    nq = gy.numel()
    ad = gy.abs()
    ev = ev_scale * 4 * U * sd_pre(xp.abs(), w9.abs(), b3.abs())
    amb = ((pre.abs() <= ev) & (ev > 0)).double()        # ev = 0: exact, the mask cannot flip
    mk, ik = f32(mean), f32(inv)
    e_xh = ev * ik + ((v - mk) * ik - xh).abs() + 2 * U * (v - mk).abs() * ik
    E_S1 = 2 * nq * D * ad.sum(dims)
    E_S2 = (ad * e_xh).sum(dims) + 2 * nq * D * (ad * xh.abs()).sum(dims)
    E_D = (ad * amb).sum(dims) + 2 * nq * D * ad.sum(dims)
    E_A = torch.einsum("bohw,bchw->oc", ad * amb, xp.abs()) + 2 * nq * D * torch.einsum("bohw,bchw->oc", ad, xp.abs())
    cb = (sum_v - mean3 * sum_m).abs()
    cw = (vx - mean3[:, None] * mx).abs()
    ga = gi.abs()
    b_gb3 = ga * (E_D + sum_m / N * E_S1 + inv3 * cb / N * E_S2) + 2 * U * gb3.abs() \
        + 8 * D * ga * (Dm.abs() + S1.abs() * sum_m / N + S2.abs() * inv3 * (sum_v.abs() + mean3.abs() * sum_m) / N)
    b_gw9 = ga[:, None] * (E_A + mx.abs() / N * E_S1[:, None] + (inv3[:, None] * cw / N) * E_S2[:, None]) + 2 * U * gw9.abs() \
        + 8 * D * ga[:, None] * (A.abs() + (S1.abs() / N)[:, None] * mx.abs()
                                 + (S2.abs() * inv3 / N)[:, None] * (vx.abs() + mean3.abs()[:, None] * mx.abs()))
    ref = dict(gw9=gw9, gb3=gb3, ggamma=S2, gbeta=S1)
    bound = dict(gw9=b_gw9, gb3=b_gb3, ggamma=2 * U * S2.abs() + E_S2, gbeta=2 * U * S1.abs() + E_S1)
    return ref, bound, int(amb.sum())
