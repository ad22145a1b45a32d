"""The float64 restatements of tests/norm_ref.py against torch in float64 (nn.BatchNorm1d, F.layer_norm, the Conv2d -> ReLU ->
BatchNorm2d -> nn.Upsample chain of BilinearModule), a float32 emulation of the BatchNorm and LayerNorm kernels inside their
bounds, and every gate rejecting its planted mistakes.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R

U = R.U


def rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def rejects(got, ref, bound):
    return R.ratio(got, ref, bound) > 1.0


def close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


# ---------------------------------------------------------------- BatchNorm
def bn_case(seed, n=600, c=12):
    g = torch.Generator().manual_seed(seed)
    x = rand(g, n, c) * 1.5 + 0.3
    return g, x, rand(g, n, c), torch.rand(c, generator=g, dtype=torch.float64) + 0.5, rand(g, c), rand(g, n, c)


@pytest.mark.parametrize("res,relu", [(False, False), (False, True), (True, True)])
def test_batch_norm_train_restatement_matches_torch(res, relu):
    g, x, r, gamma, beta, gy = bn_case(1)
    n, c = x.shape
    bn = torch.nn.BatchNorm1d(c, momentum=0.1, eps=1e-5).double().train()
    bn.running_mean.copy_(rand(g, c))
    bn.running_var.copy_(torch.rand(c, generator=g, dtype=torch.float64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    xt, rt = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    y = bn(xt) + (rt if res else 0)
    if relu:
        y = torch.relu(y)
    y.backward(gy)

    mean, var = R.bn_stats(x)
    invstd = R.bn_invstd(var, 1e-5)
    rm, rv = R.bn_running(rm0, rv0, mean, var, n, 0.1)
    close(rm, bn.running_mean)
    close(rv, bn.running_var)
    yr, _, _ = R.bn_apply(x, mean, invstd, gamma, beta, r if res else None, relu)
    close(yr, y.detach())
    out, _ = R.bn_backward(gy, x, mean, invstd, gamma, (y > 0) if relu else None)
    close(out["gx"], xt.grad)
    close(out["dgamma"], bn.weight.grad)
    close(out["dbeta"], bn.bias.grad)
    if res:
        close(out["dy"], rt.grad)


def test_batch_norm_eval_restatement_matches_torch():
    g, x, r, gamma, beta, _ = bn_case(2)
    c = x.shape[1]
    bn = torch.nn.BatchNorm1d(c, eps=1e-5).double().eval()
    with torch.no_grad():
        bn.running_mean.copy_(rand(g, c))
        bn.running_var.copy_(torch.rand(c, generator=g, dtype=torch.float64) + 0.5)
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        y = torch.relu(bn(x) + r)
    yr, _, _ = R.bn_eval(x, bn.running_mean, bn.running_var, 1e-5, gamma, beta, r, True)
    close(yr, y)


def test_batch_norm_float32_emulation_stays_inside_the_bounds():
    """The kernels' float32 steps on the CPU (no contraction): apply and backward within their bounds."""
    g, x, r, gamma, beta, gy = bn_case(3, n=4000, c=16)
    x, r, gamma, beta, gy = (R.f32(t) for t in (x, r, gamma, beta, gy))
    mean, var = R.bn_stats(x)
    mk, ik = R.f32(mean), R.f32(R.bn_invstd(var, R.f32(torch.tensor(1e-5))))
    f = lambda t: t.float()     # noqa: E731
    pre = f(f(f(x) - f(mk)) * f(ik)) * f(gamma) + f(beta) + f(r)
    y32 = torch.relu(pre)
    y, _, yb = R.bn_apply(x, mk, ik, gamma, beta, r, True)
    assert R.ratio(y32, y, yb) <= 1.0
    mask = y32 > 0
    out, b = R.bn_backward(gy, x, mk, ik, gamma, mask)
    dy = f(gy) * mask
    xh = f(f(x) - f(mk)) * f(ik)
    S0, S1 = dy.double().sum(0), (dy.double() * xh.double()).sum(0)
    inv_n = torch.tensor(1.0 / x.shape[0]).float()
    gx32 = f(gamma) * f(ik) * (dy - S0.float() * inv_n - xh * (S1.float() * inv_n))
    assert R.ratio(S0.float(), out["dbeta"], b["dbeta"]) <= 1.0
    assert R.ratio(S1.float(), out["dgamma"], b["dgamma"]) <= 1.0
    assert R.ratio(gx32, out["gx"], b["gx"]) <= 1.0


def test_batch_norm_gates_reject_planted_mistakes():
    g, x, r, gamma, beta, gy = bn_case(4, n=3000, c=16)
    n = x.shape[0]
    mean, var = R.bn_stats(x)
    invstd = R.bn_invstd(var, 1e-5)
    mb, ib = R.bn_stats_bounds(x, mean, invstd)
    row = int(torch.argmax((x - mean).abs().sum(1)))
    mean_d, var_d = R.bn_stats(x, drop_row=row)                              # one row dropped from the statistics
    assert rejects(mean_d, mean, mb) and rejects(R.bn_invstd(var_d, 1e-5), invstd, ib)
    rm0, rv0 = rand(g, 16), torch.ones(16, dtype=torch.float64)
    rm, rv = R.bn_running(rm0, rv0, mean, var, n, 0.1)
    rmb, rvb = R.bn_running_bounds(rm0, rv0, mean, var, x, 0.1)
    assert rejects(R.bn_running(rm0, rv0, mean, var, n, 0.1, unbiased=False)[1], rv, rvb)    # biased variance in running_var
    assert rejects(R.bn_running(rm0, rv0, mean_d, var, n, 0.1)[0], rm, rmb)
    y, pre, yb = R.bn_apply(x, mean, invstd, gamma, beta, r, True)
    mask = y > 0
    out, b = R.bn_backward(gy, x, mean, invstd, gamma, mask)
    flip = mask.clone()
    k = int(torch.argmax((gy * mask).abs().reshape(-1)))
    flip.view(-1)[k] = ~flip.view(-1)[k]                                     # one element's mask flipped
    out_f, _ = R.bn_backward(gy, x, mean, invstd, gamma, flip)
    assert rejects(out_f["gx"], out["gx"], b["gx"])
    assert not torch.equal(gy, out["dy"])                                    # gres unmasked
    assert not torch.equal(out_f["dy"], out["dy"])
    out_d, _ = R.bn_backward(gy, x, mean, invstd, gamma, mask, drop_row=row)
    for key in ("dbeta", "dgamma", "gx"):
        assert rejects(out_d[key], out[key], b[key]), key
    rmr, rvr = rand(g, 16) * 0.1, torch.rand(16, generator=g, dtype=torch.float64) + 0.5
    ye, _, eb = R.bn_eval(x, rmr, rvr, 1e-5, gamma, beta, r, True)
    assert rejects(R.bn_apply(x, mean, invstd, gamma, beta, r, True)[0], ye, eb)   # eval mode using batch statistics


# ---------------------------------------------------------------- add + LayerNorm
def ln_case(seed, rows=40, C=768):
    g = torch.Generator().manual_seed(seed)
    return (g, rand(g, rows, C), rand(g, rows, C), rand(g, C, scale=0.1), 1 + rand(g, C, scale=0.1), rand(g, C, scale=0.1),
            rand(g, rows, C), rand(g, rows, C))


def test_layer_norm_restatement_matches_torch():
    g, x, y, yb, w, b, gh, gs = ln_case(5)
    eps = 1e-6
    xt, yt, ybt, wt, bt = (t.clone().requires_grad_(True) for t in (x, y, yb, w, b))
    s = xt + (yt + ybt)
    h = F.layer_norm(s, (768,), wt, bt, eps)
    ((h * gh).sum() + (s * gs).sum()).backward()
    sr, _ = R.ln_sum(x, y, yb)
    mean, rstd = R.ln_stats(sr, eps)
    hr, _ = R.ln_apply(sr, mean, rstd, w, b)
    close(sr, s.detach())
    close(hr, h.detach())
    out, _ = R.ln_backward(gh, gs, sr, w, mean, rstd, 3, 1)
    close(out["gx"], xt.grad)
    close(out["gx"], yt.grad)
    close(R.ln_colsum(out["gx"], 1)[0], ybt.grad)
    close(out["dgamma"], wt.grad)
    close(out["dbeta"], bt.grad)


def test_layer_norm_float32_emulation_stays_inside_the_bounds():
    g, x, y, yb, w, b, gh, gs = ln_case(6, rows=64)
    x, y, yb, w, b, gh, gs = (R.f32(t) for t in (x, y, yb, w, b, gh, gs))
    f = lambda t: t.float()     # noqa: E731
    s32 = f(x) + (f(y) + f(yb))
    sr, sb = R.ln_sum(x, y, yb)
    assert R.ratio(s32, sr, sb) <= 1.0
    s = s32.double()
    m32 = s32.sum(1) * torch.tensor(1 / 768).float()
    mean, _ = R.ln_stats(s, 1e-6)
    _, rstd = R.ln_stats(s, 1e-6, m32.double())
    mb, rb = R.ln_stats_bounds(s, rstd, 3)
    r32 = torch.rsqrt(((s32 - m32[:, None]) ** 2).sum(1) * torch.tensor(1 / 768).float() + 1e-6)
    assert R.ratio(m32, mean, mb) <= 1.0 and R.ratio(r32, rstd, rb) <= 1.0
    mk, rk = m32.double(), r32.double()
    h, hb = R.ln_apply(s, mk, rk, w, b)
    assert R.ratio((s32 - m32[:, None]) * r32[:, None] * f(w) + f(b), h, hb) <= 1.0
    out, bb = R.ln_backward(gh, gs, s, w, mk, rk, 3, 4)
    xh = (s32 - m32[:, None]) * r32[:, None]
    gy = f(gh) * f(w)
    c1 = gy.sum(1, keepdim=True) * torch.tensor(1 / 768).float()
    c2 = (gy * xh).sum(1, keepdim=True) * torch.tensor(1 / 768).float()
    gx32 = r32[:, None] * (gy - c1 - xh * c2) + f(gs)
    assert R.ratio(gx32, out["gx"], bb["gx"]) <= 1.0


def test_layer_norm_gates_reject_planted_mistakes():
    g, x, y, yb, w, b, gh, gs = ln_case(7)
    s, _ = R.ln_sum(x, y, yb)
    mean, rstd = R.ln_stats(s, 1e-6)
    mb, rb = R.ln_stats_bounds(s, rstd, 3)
    j = int(torch.argmax(s.abs().sum(0)))
    assert rejects(R.ln_stats(s, 1e-6, drop_col=j)[0], mean, mb)       # a row mean missing one element
    assert rejects(R.ln_stats(s, 1e-6, mean, ddof=1)[1], rstd, rb)      # variance over C - 1
    out, bb = R.ln_backward(gh, gs, s, w, mean, rstd, 3, 4)
    out_n, _ = R.ln_backward(gh, gs, s, w, mean, rstd, 3, 4, add_gs=False)
    assert rejects(out_n["gx"], out["gx"], bb["gx"])                   # gs not added
    ref, cb = R.ln_colsum(out["gx"], 4)
    assert rejects(R.ln_colsum(out_n["gx"], 4)[0], ref, cb)


# ---------------------------------------------------------------- sample-down
def sd_case(seed, B=2, H=37, W=53, oh=48, ow=24):
    g = torch.Generator().manual_seed(seed)
    w9, b3 = R.dyadic_params(g)
    img = R.plant_zeros(R.dyadic_image(g, B, H, W), w9, b3, oh, ow, per_channel=6, seed=seed)
    gamma, beta = torch.tensor([1.3, 0.7, 1.1], dtype=torch.float64), torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64)
    gy = torch.randint(-64, 65, (B, 3, oh, ow), generator=g).double() / 64
    return img, w9, b3, gamma, beta, gy


def sd_saved(img, w9, b3, eps, mask_ge=False):
    n = img.numel() // 3
    sums = R.sd_forward_sums(img, w9, b3, mask_ge)
    mean, var, inv = R.sd_stats(sums, n, eps)
    return torch.cat([sums, mean, inv]), var, n


def test_sample_down_restatement_matches_torch_modules():
    img, w9, b3, gamma, beta, gy = sd_case(8)
    oh, ow = gy.shape[2:]
    mod = torch.nn.Sequential(torch.nn.Conv2d(3, 3, 1), torch.nn.ReLU(), torch.nn.BatchNorm2d(3), torch.nn.Upsample((oh, ow))).double().train()
    with torch.no_grad():
        mod[0].weight.copy_(w9.view(3, 3, 1, 1))
        mod[0].bias.copy_(b3)
        mod[2].weight.copy_(gamma)
        mod[2].bias.copy_(beta)
    yo = mod(img)
    yo.backward(gy)
    saved, var, n = sd_saved(img, w9, b3, 1e-5)
    assert R.sd_pick_index(img.shape[2], img.shape[3], oh, ow)[0].unique().numel() < oh      # rows picked twice
    out, _ = R.sd_out(R.sd_picked(img, oh, ow), w9, b3, saved[27:30], saved[30:33], gamma, beta)
    close(out, yo.detach())
    rm, rv = R.bn_running(torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64), saved[27:30], var, n, 0.1)
    close(rm, mod[2].running_mean)
    close(rv, mod[2].running_var)
    ref, _, _ = R.sd_backward(img, gy, w9, b3, gamma, saved, n)
    close(ref["gw9"], mod[0].weight.grad.view(3, 3))
    close(ref["gb3"], mod[0].bias.grad)
    close(ref["ggamma"], mod[2].weight.grad)
    close(ref["gbeta"], mod[2].bias.grad)


def test_sample_down_eval_restatement_matches_torch_modules():
    img, w9, b3, gamma, beta, _ = sd_case(9)
    bn = torch.nn.BatchNorm2d(3).double().eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.tensor([0.2, 0.5, 0.1]))
        bn.running_var.copy_(torch.tensor([0.7, 1.5, 0.4]))
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        yo = F.interpolate(bn(torch.relu(R.sd_pre(img, w9, b3))), size=(48, 24))
    out, _ = R.sd_out(R.sd_picked(img, 48, 24), w9, b3, bn.running_mean, R.bn_invstd(bn.running_var, 1e-5), gamma, beta)
    close(out, yo)


def test_sample_down_gates_reject_planted_mistakes():
    img, w9, b3, gamma, beta, gy = sd_case(10)
    saved, var, n = sd_saved(img, w9, b3, 1e-5)
    ref, bound, amb = R.sd_backward(img, gy, w9, b3, gamma, saved, n, ev_scale=0.0)
    assert amb == 0
    saved_ge, _, _ = sd_saved(img, w9, b3, 1e-5, mask_ge=True)
    assert not torch.equal(saved_ge[6:18], saved[6:18])
    mutants = {"m = (v >= 0)": R.sd_backward(img, gy, w9, b3, gamma, saved_ge, n, mask_ge=True, ev_scale=0.0)[0],
               "N = picked pixels": R.sd_backward(img, gy, w9, b3, gamma, saved, n, n_picked=True, ev_scale=0.0)[0],
               "S2 term dropped": R.sd_backward(img, gy, w9, b3, gamma, saved, n, drop_s2=True, ev_scale=0.0)[0],
               "second pick dropped": R.sd_backward(img, gy, w9, b3, gamma, saved, n, drop_dup=True, ev_scale=0.0)[0]}
    for name, mut in mutants.items():
        assert rejects(mut["gw9"], ref["gw9"], bound["gw9"]) and rejects(mut["gb3"], ref["gb3"], bound["gb3"]), name
    # eval mode using batch statistics
    rm, rv = torch.tensor([0.2, 0.5, 0.1], dtype=torch.float64), torch.tensor([0.7, 1.5, 0.4], dtype=torch.float64)
    xp = R.sd_picked(img, 48, 24)
    ye, eb = R.sd_out(xp, w9, b3, rm, R.bn_invstd(rv, 1e-5), gamma, beta)
    assert rejects(R.sd_out(xp, w9, b3, saved[27:30], saved[30:33], gamma, beta)[0], ye, eb)
    # the forward sums: the mask's strictness shows in sum m and sum m x_c, which are exact here
    assert rejects(saved_ge[:27], saved[:27], torch.zeros(27, dtype=torch.float64))


def test_sample_down_forward_sum_bounds_cover_a_float32_emulation():
    g = torch.Generator().manual_seed(11)
    img = R.f32(torch.randn(2, 3, 40, 50, generator=g, dtype=torch.float64))
    w9, b3 = R.f32(torch.randn(3, 3, generator=g, dtype=torch.float64) * 0.5), R.f32(torch.randn(3, generator=g, dtype=torch.float64) * 0.1)
    ref = R.sd_forward_sums(img, w9, b3)
    e, amb = R.sd_forward_sum_bounds(img, w9, b3)
    f = img.float()
    pre32 = torch.einsum("oc,bchw->bohw", w9.float(), f) + b3.float().view(1, 3, 1, 1)
    v = pre32.clamp_min(0).double()
    m = (pre32 > 0).double()
    got = torch.cat([v.sum((0, 2, 3)), (v * v).sum((0, 2, 3)), m.sum((0, 2, 3)), torch.einsum("bohw,bchw->oc", m, img).reshape(9),
                     torch.einsum("bohw,bchw->oc", v, img).reshape(9)])
    assert R.ratio(got, ref, e + 1e-300) <= 1.0
    assert np.all(amb.numpy() < 5)
