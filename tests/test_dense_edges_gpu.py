"""The dense MFMA GEMM families (ftx_dense_gemm_*, ftx_dense_wgrad_*, ftx_vit_patch_embed_*, ftx_vit_tap_stem_*) against float64 at
every tile and split edge of tests/dense_edges.py: the last row tile at every sub-tile border, column tails in both weight orientations,
every epilogue at a tail, k = 64, every split count with short, odd and one-row last splits, n and k tails of the weight gradient, and
the two forms at every tile.  The gates are those of tests/test_vit_linear_bf16_gpu.py and tests/test_vit_linear_split_gpu.py
(dense_edges.py's docstring); every output lies between guard bands (tests/guard.py), so a wrong address shows as well as a wrong value.

Every test prints one EDGE line: the worst error / bound per output (and E / T of gate G2 for the split family).  Those lines are the
record kept in profiles/dense_edges.txt; they are figures, not gates."""
import numpy as np
import pytest
import torch

from tests import dense_edges as E
from tests import guard as GD

pytestmark = pytest.mark.gpu
U = E.U
EPS = float(np.float32(1e-5))
DEV = "cuda"


@pytest.fixture(scope="module")
def env():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return spf, _lib.load()


# ---------------------------------------------------------------- guarded calls of the C entries
class Out:
    """An output between guard bands, the sentinel (a NaN) everywhere: 16-byte aligned and no more, as the guard-band tests place it."""

    def __init__(self, shape):
        self.whole, self.view = GD.banded(shape, band=GD.dense_band(shape), device=DEV)
        self.address = GD.address(self.whole, self.view)

    def checked(self, what):
        assert GD.bands_intact(self.whole, self.view), (what, "a guard band was written")
        assert GD.written(self.view), (what, "an element was not written, or is not finite")
        return self.view


def call(env, name, *args):
    spf, L = env
    spf.check(getattr(L, name)(*args, spf.stream()), name)
    torch.cuda.synchronize()


def c_gemm(env, family, a, w, w_kn, epi, bias=None, pre_in=None, with_pre=False):
    spf, L = env
    m, k = a.shape
    n = w.shape[1] if w_kn else w.shape[0]
    out, pre = Out((m, n)), (Out((m, n)) if with_pre else None)
    call(env, "ftx_dense_gemm_" + family, a.data_ptr(), w.data_ptr(), w_kn, spf.ptr(bias), spf.ptr(pre_in), m, n, k, epi, out.address,
         pre.address if with_pre else 0)
    what = (family, m, n, k, w_kn, epi)
    # the package's own wrapper admits every shape the entry admits: the same bits through it
    lib_out, lib_pre = spf._dense_gemm(a, w, w_kn, epi, bias=bias, pre_in=pre_in, with_pre=with_pre, mode=family)
    assert GD.same_bits(out.checked(what), lib_out), what
    if with_pre:
        assert GD.same_bits(pre.checked(what), lib_pre), what
    return out.view, (pre.view if with_pre else None)


def c_wgrad(env, family, dy, x, splits):
    spf, L = env
    (m, n), k = dy.shape, x.shape[1]
    ws_bytes = int(getattr(L, f"ftx_dense_wgrad_{family}_workspace_bytes")(m, n, k))
    assert ws_bytes == max(256, 4 * splits * n * k if splits > 1 else 0)
    ws_whole, ws = GD.banded_bytes(ws_bytes, device=DEV)       # exactly the queried size, poisoned, between bands
    dw = Out((n, k))
    call(env, "ftx_dense_wgrad_" + family, dy.data_ptr(), x.data_ptr(), m, n, k, dw.address, GD.address(ws_whole, ws), ws_bytes)
    what = (family, m, n, k, splits)
    assert GD.bands_intact(ws_whole, ws), (what, "the workspace was used beyond the size its query returns")
    assert splits > 1 or GD.sentinel_only(ws), (what, "an unsplit weight gradient touches no workspace")
    assert GD.same_bits(dw.checked(what), spf._dense_wgrad(dy, x, family)), what
    return dw.view


class Gate:
    """The per-element gate on one test's outputs, keeping worst error / bound of each for the record."""

    def __init__(self):
        self.figures = []

    def __call__(self, what, out, ref, bound):
        r = E.worst(out, ref, bound)
        self.figures.append(f"{what} {r:.3g}")
        assert E.passes(out, ref, bound), (what, r)

    def g2(self, what, out, parts, add=None):
        e, t = E.g2_figures(out, parts, add)
        self.figures.append(f"{what} E/T {e / t:.3g}")
        assert out.numel() < E.G2_MIN_ELEMS or e <= t / 2, (what, e, t)      # an rms statistic: printed only below G2_MIN_ELEMS

    def record(self, head):
        print(f"\nEDGE {head}: " + "  ".join(self.figures))


def _id(case):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in case)


# ---------------------------------------------------------------- the plain GEMM
def run_gemm(env, family, case, gate):
    """Every epilogue of both weight orientations at one case, gated; returns what the fault test needs."""
    spf, L = env
    m, n, k, tile, rt, ct = case
    assert spf.dense_tile(family, 0, m, n, k) == tile + (1,)
    x, w, b = E.data(m, k, n, seed=m * 7 + k + n, device=DEV)
    b_kn = w.t().contiguous()
    s, sa = E.gemm_ref(family, x, b_kn)
    f = E.factor(family, k)
    parts = E.g2_parts(x, b_kn) if family == "split" else None
    # W stored [N][K]: NONE, BIAS, BIAS_GELU
    none, _ = c_gemm(env, family, x, w, 0, spf.EPI_NONE)
    gate("NONE", none, s, f * U * sa)
    bias, _ = c_gemm(env, family, x, w, 0, spf.EPI_BIAS, bias=b)
    pre_ref, pre_bound = E.bias_ref(s, sa, b, f)
    gate("BIAS", bias, pre_ref, pre_bound)
    h, pre = c_gemm(env, family, x, w, 0, spf.EPI_BIAS_GELU, bias=b, with_pre=True)
    assert GD.same_bits(pre, bias), "the pre-activation is the BIAS epilogue's output"
    gate("BIAS_GELU", h, *E.gelu_ref(pre_ref, pre_bound, pre))
    # W stored [K][N]: NONE, DGELU
    dx, _ = c_gemm(env, family, x, b_kn, 1, spf.EPI_NONE)
    gate("kn NONE", dx, s, f * U * sa)
    pre_in = E.randn((m, n), m + 2, DEV, 2.0)
    dp, _ = c_gemm(env, family, x, b_kn, 1, spf.EPI_DGELU, pre_in=pre_in)
    gate("kn DGELU", dp, *E.dgelu_ref(s, sa, pre_in, f))
    if family == "split":
        gate.g2("NONE", none, parts)
        gate.g2("BIAS", bias, parts, b)
        gate.g2("kn NONE", dx, parts)
    return dict(x=x, b_kn=b_kn, b=b, s=s, sa=sa, f=f, bias=bias, dx=dx, pre_bound=pre_bound)


@pytest.mark.parametrize("case", E.GEMM_CASES, ids=_id)
@pytest.mark.parametrize("family", E.FAMILIES)
def test_gemm_edges(env, family, case):
    gate = Gate()
    try:
        run_gemm(env, family, case, gate)
    finally:
        gate.record("gemm %s m=%d n=%d k=%d tile=%dx%d rows=%d cols=%d" % ((family,) + case[:3] + case[3] + case[4:]))


# ---------------------------------------------------------------- the weight gradient
def run_wgrad(env, family, case, gate):
    spf, L = env
    m, n, k, splits, last = case
    assert spf.dense_tile(family, 1, m, n, k) == (128, 128, splits)
    dy, x = E.randn((m, n), m + 1, DEV, 0.1), E.randn((m, k), m * 7 + n + k, DEV)
    dw = c_wgrad(env, family, dy, x, splits)
    gt = dy.t().contiguous()
    s, sa = E.gemm_ref(family, gt, x)
    bound = E.wgrad_factor(family, m, splits) * U * sa
    gate("dW", dw, s, bound)
    if family == "split":
        gate.g2("dW", dw, E.g2_parts(gt, x))
    return dict(dy=dy, x=x, dw=dw, bound=bound)


@pytest.mark.parametrize("case", E.WGRAD_CASES, ids=_id)
@pytest.mark.parametrize("family", E.FAMILIES)
def test_wgrad_edges(env, family, case):
    gate = Gate()
    try:
        run_wgrad(env, family, case, gate)
    finally:
        gate.record("wgrad %s m=%d n=%d k=%d splits=%d last=%d" % ((family,) + case))


# ---------------------------------------------------------------- the forms
def run_patch(env, family, case, gate):
    spf, L = env
    b, side, dim, t0, tile, rt = case
    c, p = E.PATCH_C, E.PATCH_P
    g, k = (side // p) ** 2, c * p * p
    assert spf.dense_tile(family, 0, b * g, dim, k) == tile + (1,)
    seed = 100 * b + dim + t0
    img = E.randn((b, c, side, side), seed, DEV)
    w, bias = E.randn((dim, k), seed + 1, DEV, 0.02), E.randn((dim,), seed + 2, DEV, 0.1)
    cls, pos = E.randn((dim,), seed + 3, DEV, 0.02), E.randn((t0 + g, dim), seed + 4, DEV, 0.02)
    dist = E.randn((dim,), seed + 5, DEV, 0.02) if t0 == 2 else None
    tokens = Out((b, t0 + g, dim))
    call(env, "ftx_vit_patch_embed_" + family, img.data_ptr(), w.data_ptr(), bias.data_ptr(), cls.data_ptr(), spf.ptr(dist), pos.data_ptr(), b, c,
         side, side, p, dim, t0, tokens.address)
    out = tokens.checked(("patch embed", family) + case)
    ref, bound, a, add = E.patch_ref(family, img, w, bias, pos, t0, E.factor(family, k))
    rows = out[:, t0:].reshape(b * g, dim)
    gate("patches", rows, ref, bound)
    if family == "split":
        gate.g2("patches", rows, E.g2_parts(a, w.t()), add)
    # the rows in front are one fp32 addition: exact
    assert GD.same_bits(out[:, 0], (cls + pos[0]).expand(b, dim)), "class token rows"
    assert t0 == 1 or GD.same_bits(out[:, 1], (dist + pos[1]).expand(b, dim)), "distillation token rows"
    # and, as tests/test_native_image_gpu.py has it at the model's shapes, the bits of the plain entry on a materialised A
    y, _ = spf._dense_gemm(a, w, 0, spf.EPI_BIAS, bias=bias, mode=family)
    assert GD.same_bits(out[:, t0:], y.view(b, g, dim) + pos[t0:].unsqueeze(0)), "the form differs from the plain entry on the unfold"
    return dict(a=a, w=w, bias=bias, pos=pos, g=g, t0=t0, rows=rows, bound=bound)


@pytest.mark.parametrize("case", E.PATCH_CASES, ids=_id)
@pytest.mark.parametrize("family", E.FAMILIES)
def test_patch_embed_edges(env, family, case):
    gate = Gate()
    try:
        run_patch(env, family, case, gate)
    finally:
        gate.record("patch %s b=%d side=%d dim=%d t0=%d tile=%dx%d rows=%d" % ((family,) + case[:4] + case[4] + case[5:]))


def run_tap(env, family, case, gate):
    spf, L = env
    b, g, t0, co, tile, rt = case
    dim = E.TAP_DIM
    assert spf.dense_tile(family, 0, b * g, co, dim) == tile + (1,)
    seed = 10 * b + g + t0 + co
    tokens = E.randn((b, t0 + g, dim), seed, DEV)
    w, bias = E.randn((co, dim), seed + 1, DEV, 0.05), E.randn((co,), seed + 2, DEV, 0.5)
    gamma, beta = E.randn((co,), seed + 3, DEV).abs() + 0.5, E.randn((co,), seed + 4, DEV, 0.2)
    mean, var = E.randn((co,), seed + 5, DEV, 0.3), E.randn((co,), seed + 6, DEV).abs() + 0.5
    o = Out((b * g, co))
    call(env, "ftx_vit_tap_stem_" + family, tokens.data_ptr(), w.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
         var.data_ptr(), EPS, b, g, t0, dim, co, o.address)
    out = o.checked(("tap stem", family) + case)
    bn = (gamma, beta, mean, var, EPS)
    f = E.factor(family, dim)
    ref, bound = E.tap_ref(family, tokens, w, bias, *bn, t0, f)
    gate("tap", out, ref, bound)
    a = tokens[:, t0:].contiguous().view(b * g, dim)
    y, _ = spf._dense_gemm(a, w, 0, spf.EPI_BIAS, bias=bias, mode=family)
    with torch.no_grad():
        plain = spf.batch_norm(torch.relu(y), gamma, beta, mean, var, False, 0.1, EPS)
    assert GD.same_bits(out, plain), "the form differs from the plain entry, ReLU and eval BatchNorm on the stripped tokens"
    return dict(tokens=tokens, w=w, bias=bias, bn=bn, t0=t0, f=f, out=out, bound=bound)


@pytest.mark.parametrize("case", E.TAP_CASES, ids=_id)
@pytest.mark.parametrize("family", E.FAMILIES)
def test_tap_stem_edges(env, family, case):
    gate = Gate()
    try:
        run_tap(env, family, case, gate)
    finally:
        gate.record("tap %s b=%d g=%d t0=%d co=%d tile=%dx%d rows=%d" % ((family,) + case[:4] + case[4] + case[5:]))


# ---------------------------------------------------------------- the gates tell, on the kernels' own output
def _rejects(out, ref, bound, faults, want, what):
    assert sorted(faults) == want, (what, sorted(faults))
    assert E.passes(out, ref, bound), what
    for name, r in faults.items():
        assert not E.passes(out, r, bound), (what, "fault (%s) passes the gate" % name)


@pytest.mark.parametrize("family", E.FAMILIES)
def test_gates_reject_edge_faults(env, family):
    gate = Gate()
    # plain GEMM, both orientations: 64 x 128 tile, 33 rows in the last row tile, 68 columns in the last column tile
    case = next(c for c in E.GEMM_CASES if c[3] == (64, 128) and c[4] == 33 and c[5] == 68)
    r = run_gemm(env, family, case, gate)
    a64, b64 = E.operands64(family, r["x"], r["b_kn"])
    _rejects(r["bias"], r["s"] + r["b"].double(), r["pre_bound"], E.mutants("gemm", a=a64, b_kn=b64, bias=r["b"].double(), col_tail=case[5]),
             ["c", "d", "f"], "BIAS")
    _rejects(r["dx"], r["s"], r["f"] * U * r["sa"], E.mutants("dx", a=a64, b_kn=b64), ["c", "d", "e"], "kn NONE")
    # weight gradient: eight splits, the last of one row
    case = (2241, 68, 68, 8, 1)
    assert case in E.WGRAD_CASES
    r = run_wgrad(env, family, case, gate)
    g64, x64 = E.operands64(family, r["dy"], r["x"])
    _rejects(r["dw"], g64.t() @ x64, r["bound"], E.mutants("wgrad", g=g64, x=x64, split_len=E.wgrad_splits(*case[:3])[1]), ["a", "b"], "dW")
    # patch embedding: frame borders inside 64 x 128 tiles
    case = E.PATCH_CASES[3]
    r = run_patch(env, family, case, gate)
    a64, w64 = E.operands64(family, r["a"], r["w"].t())
    faults = E.mutants("patch", a=a64, b_kn=w64, bias=r["bias"].double(), pos=r["pos"].double(), g=r["g"], t0=r["t0"])
    ref = a64 @ w64 + r["bias"].double() + r["pos"].double()[r["t0"]:].repeat(case[0], 1)
    _rejects(r["rows"], ref, r["bound"], faults, ["g"], "patch embed")
    # tap stem with leading tokens to skip
    case = E.TAP_CASES[4]
    assert case[2] == 2
    r = run_tap(env, family, case, gate)
    ref = E.tap_ref(family, r["tokens"], r["w"], r["bias"], *r["bn"], r["t0"], r["f"])[0]
    unskipped = E.tap_ref(family, r["tokens"], r["w"], r["bias"], *r["bn"], r["t0"], r["f"], skip=False)[0]
    _rejects(r["out"], ref, r["bound"], E.mutants("tap", ref_unskipped=unskipped), ["h"], "tap stem")


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("family", E.FAMILIES)
def test_edges_are_deterministic(env, family):
    spf, L = env
    m, n, k, tile, rt, ct = next(c for c in E.GEMM_CASES if c[3] == (128, 128) and c[4] == 97 and c[5] == 68)
    x, w, b = E.data(m, k, n, 3, DEV)
    b_kn = w.t().contiguous()
    pre_in = E.randn((m, n), 4, DEV, 2.0)
    dy, xr = E.randn((2241, 68), 5, DEV, 0.1), E.randn((2241, 68), 6, DEV)
    assert spf.dense_tile(family, 1, 2241, 68, 68)[2] == 8

    def run():
        return (c_gemm(env, family, x, w, 0, spf.EPI_BIAS_GELU, bias=b, with_pre=True) + c_gemm(env, family, x, b_kn, 1, spf.EPI_DGELU, pre_in=pre_in)[:1]
                + (c_wgrad(env, family, dy, xr, 8),))

    first, again = run(), run()
    assert len(first) == 4 and all(GD.same_bits(a, e) for a, e in zip(first, again))
